"""The dense engine's fp32 (parity) kernels alone through the C ABI: rpc_dense_conv_f32 on all six maps,
rpc_dense_wgrad_f32, rpc_dense_wprep_batch_f32 and the fp32 BatchNorm passes, element by element against the float64
references of tests/_dense_cases.py.

Operands are full 24-bit fp32 random values, not a coarse grid: an engine that truncated them must fail. u = 2^-24.

Bounds, derived from the arithmetic and not from what the kernels give:
    conv      every stored element within (n + 8) u mag of float64, n = taps * cin (+ 1 with accumulate), mag =
              sum |a| |w| (+ |base|): every product rounded once, summed in fp32 in any order. At cin = 16 .. 64
              this lies below the error of operands cut to bf16 or tf32 (2^-9 / 2^-11 per operand against about
              2^-24 (n + 8) / sqrt(n) of a random-sign sum).
    partials  row par * nblk + b = column sums and sums of squares of the values stored for GEMM rows 64b .. 64b + 63
              of parity par, within 72 u of their magnitudes (64 additions, the square, reading back the stored
              value is exact); one more sentinel row stays untouched. With accumulate: of the values after the add.
    wgrad     (n_t + 8) u mag, n_t = rows whose tap t lies inside the image. The slab reduction adds no term:
              k_wgrad_reduce sums the fp32 slabs in double (chunks * 2^-53, far below u) and rounds once to fp32,
              which the + 8 covers; the slabs' own fp32 sums have n_c terms each with sum n_c = n_t.
    wprep     bit for bit a permutation.
    BatchNorm as in test_gpu_dense_bn_passes.py with fp32 images (no 2^-8 term); the double partial rows of
              rpc_dense_bnbwd_stats_f32 each within (M + 8) 2^-53 of their own terms' magnitudes; the chain stats ->
              rpc_bn_finalize(mode 1 | RPC_BN_PART_F64) -> apply within 8 u mag of bnbwd_apply_ref fed the bnb the
              kernels wrote (rpc_bn_finalize has its own float64 test, test_dense_cases_cpu.py ties the formulas to
              autograd).

Measured on the MI355X (the module prints them when it ends; 183 tests in 5 s): worst err / tol per entry
    rpc_dense_conv_f32        S1 0.025  flipped S1 0.034  S2 0.027  D2 0.028  P1 0.15  U2 0.19  G2 0.056
                              partial rows 0.034 .. 0.041 on every map
    rpc_dense_wgrad_f32       S1 0.16  S2 0.15  P1 0.11  U2 0.11
    rpc_dense_bn_apply_f32    0.48     rpc_dense_bnbwd_apply_f32 0.39     chain 0.39
    rpc_dense_bnbwd_stats_f32 totals below 0.0001 of the fp32 bound; rows 0.17 of the 2^-53 bound
No case misses its bound, so no step is added to one. No kernel bug was found.
Mutants that stay in bounds, one build and one run of this module each: k_igemm_f32 without the sr < 0 zeroing
(border taps read row 0) fails test_conv_f32_matches_fp64 on S1, flipped S1, S2 and D2 (28 of 46); its staged
operands cut to bf16 precision fail all 46; s2 summed before the accumulate add fails all 46 (the partial rows of
the accumulate way); k_wgrad_f32 with rb1 one row short fails all 24 of test_wgrad_f32_matches_fp64.
"""
import pytest
import torch

from robustpointclouds_amd import _ffi
from tests import _dense_cases as dc
from tests import test_gpu_dense_bn_passes as bp

pytestmark = pytest.mark.gpu

U = dc.U
SPARE = 3
WORST = {}
F32 = bp.F32
within, gen, raw = bp.within, bp.gen, bp.raw
MAPS = [dc.S1, dc.FS1, dc.S2, dc.D2, dc.P1, dc.U2, dc.G2]
CONV_CASES = [(m, i) for m in MAPS for i in range(len(dc.conv_cases(m, dc.IMAGES_F32)))]
WGRAD_MAPS = [dc.S1, dc.S2, dc.P1, dc.U2]


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    bp.report(WORST)


def _dev():
    return torch.device("cuda")


def _conv(lib, fmap, xd, sp, cin, wd, cout, out, op, ooff, accum, part, R, S, O):
    _ffi.check(lib.rpc_dense_conv_f32(dc.ABI_MAP[fmap], _ffi.ptr(xd), sp, cin, _ffi.ptr(wd), cout, _ffi.ptr(out), op,
                                      ooff, accum, _ffi.ptr(part), _ffi.int_arr(R), _ffi.int_arr(S), _ffi.int_arr(O),
                                      _ffi.stream_of(out)), "rpc_dense_conv_f32")
    torch.cuda.synchronize()


def _check_part(part, fmap, R, O, got, what, entry):
    """partial rows [npar * nblk + 1][2C] against the stored values, 64 GEMM rows of one parity per row"""
    Cc = got.shape[1]
    nblk = (dc.npix(R) + 63) // 64
    npar = 4 if fmap == dc.U2 else 1
    assert part.shape[0] == npar * nblk + 1 and torch.isnan(part[npar * nblk]).all(), what
    p = part[:npar * nblk].cpu().double()
    for par in range(npar):
        v = got[dc.out_rows(R, O, par)] if fmap == dc.U2 else got
        s1, a1 = dc.tile_sums(v, 64)
        s2, a2 = dc.tile_sums(v * v, 64)
        rows = p[par * nblk:(par + 1) * nblk]
        within(rows[:, :Cc], s1, 72 * U * a1, what + f" part[0] par {par}", entry + " part", WORST)
        within(rows[:, Cc:], s2, 72 * U * a2, what + f" part[1] par {par}", entry + " part", WORST)


# ------------------------------------------------------------------ rpc_dense_conv_f32
@pytest.mark.parametrize("fmap,idx", CONV_CASES)
def test_conv_f32_matches_fp64(fmap, idx):
    lib = _ffi.load()
    dev = _dev()
    R, S, O = dc.conv_cases(fmap, dc.IMAGES_F32)[idx]
    Mo, T = dc.npix(O), dc.TAPS[fmap]
    nb = lib.rpc_dense_conv_blocks_f32(dc.ABI_MAP[fmap], _ffi.int_arr(R))
    assert nb == (dc.npix(R) + 63) // 64 * (4 if fmap == dc.U2 else 1)
    entry = "conv_f32 " + dc.MAP_NAMES[fmap]
    for cin, cout in dc.CHANNELS_F32:
        g = gen("conv_f32", fmap, R, S, cin, cout)
        x = torch.randn((dc.npix(S), cin), generator=g)
        W = torch.randn(dc.layer_weight_shape(fmap, cin, cout), generator=g) * 0.1
        base = torch.randn((Mo, cout), generator=g)
        ref, mag = dc.conv_ref(fmap, x, W, dc.KIND[fmap], R, S, O)
        wd = dc.gemm_weights(fmap, W).to(dev)
        n = T * cin
        ways = [("dense", cin, cout, 0, 0), ("pitched", cin + 16, 2 * cout + 8, cout + 8, 0),
                ("accumulate", cin, cout, 0, 1)]
        for way, sp, op, ooff, accum in ways:
            what = f"{entry} {R} <- {S} ({cin},{cout}) {way}"
            xd = dc.pack(x, sp, 0).to(dev)
            out = dc.pack(base, op, ooff, SPARE) if accum else dc.sentinel_buffer(Mo + SPARE, op, torch.float32)
            out = out.to(dev)
            part = torch.full((nb + 1, 2 * cout), float("nan"), device=dev)
            _conv(lib, fmap, xd, sp, cin, wd, cout, out, op, ooff, accum, part, R, S, O)
            assert dc.outside_unchanged(out, Mo, cout, ooff), what
            got = dc.unpack(out, Mo, cout, ooff).cpu().double()
            if accum:
                within(got, ref + base.double(), (n + 9) * U * (mag + base.double().abs()), what, entry, WORST)
            else:
                within(got, ref, (n + 8) * U * mag, what, entry, WORST)
            _check_part(part, fmap, R, O, got, what, entry)
            if way == "dense":                                   # part = NULL: the same image
                out2 = dc.sentinel_buffer(Mo + SPARE, op, torch.float32).to(dev)
                _conv(lib, fmap, xd, sp, cin, wd, cout, out2, op, ooff, 0, None, R, S, O)
                assert torch.equal(raw(out2), raw(out)), what
        if dc.npix(R) > 1 and fmap not in (dc.P1, dc.U2, dc.G2):
            assert (dc.src_rows(fmap, R, S) < 0).any()           # the case has taps without a source


def test_conv_f32_argument_guards():
    lib = _ffi.load()
    dev = _dev()
    img = (1, 4, 4)
    x = torch.zeros((16, 64), device=dev)
    w = torch.zeros((9, 64, 64), device=dev)
    out = dc.sentinel_buffer(16, 136, torch.float32).to(dev)
    part = torch.full((2, 128), float("nan"), device=dev)
    P, ia, st = _ffi.ptr, _ffi.int_arr, _ffi.stream_of(x)

    def conv(fmap=0, sp=64, cin=64, cout=64, op=64, ooff=0):
        return lib.rpc_dense_conv_f32(fmap, P(x), sp, cin, P(w), cout, P(out), op, ooff, 0, P(part), ia(img), ia(img),
                                      ia(img), st)

    assert conv(cin=8) == dc.RPC_ERR_ARG and conv(cin=24, sp=24) == dc.RPC_ERR_ARG          # cin % 16
    assert conv(cout=32) == dc.RPC_ERR_ARG and conv(cout=96, op=96) == dc.RPC_ERR_ARG       # cout % 64
    assert conv(sp=48) == dc.RPC_ERR_ARG                                                   # src_pitch < cin
    assert conv(op=60) == dc.RPC_ERR_ARG and conv(op=72, ooff=12) == dc.RPC_ERR_ARG         # out_pitch < offset + cout
    assert conv(sp=66) == dc.RPC_ERR_ARG and conv(op=70) == dc.RPC_ERR_ARG                  # not multiples of 4
    assert conv(op=134, ooff=70) == dc.RPC_ERR_ARG and conv(op=136, ooff=70) == dc.RPC_ERR_ARG
    assert conv(fmap=-1) == dc.RPC_ERR_ARG and conv(fmap=6) == dc.RPC_ERR_ARG               # map out of range
    torch.cuda.synchronize()
    assert dc.is_sentinel(out).all() and torch.isnan(part).all()


# ------------------------------------------------------------------ rpc_dense_wgrad_f32
def _wgrad(lib, fmap, kind, xd, xp, ci, dd, dp, co, R, S, O, dW, ws, wsz):
    return lib.rpc_dense_wgrad_f32(fmap, kind, _ffi.ptr(xd), xp, ci, _ffi.ptr(dd), dp, co, _ffi.int_arr(R),
                                   _ffi.int_arr(S), _ffi.int_arr(O), _ffi.ptr(dW), _ffi.ptr(ws), wsz,
                                   _ffi.stream_of(dW))


@pytest.mark.parametrize("img", dc.WGRAD_IMAGES_F32)
@pytest.mark.parametrize("fmap", WGRAD_MAPS)
def test_wgrad_f32_matches_fp64(fmap, img):
    lib = _ffi.load()
    dev = _dev()
    R, S, O = dc.wgrad_geometry(fmap, img)
    kind = dc.KIND[fmap]
    entry = "wgrad_f32 " + dc.MAP_NAMES[fmap]
    for ci, co in dc.WGRAD_CHANNELS:
        what = f"{entry} {R} ({ci},{co})"
        g = gen("wgrad_f32", fmap, img, ci, co)
        x = torch.randn((dc.npix(S), ci), generator=g)
        dz = torch.randn((dc.npix(O), co), generator=g)
        ref, mag = dc.wgrad_ref(fmap, x, dz, kind, R, S, O)
        nt = dc.wgrad_bound_terms(fmap, kind, R, S, ref.shape)
        xp, dp = ci + 16, co + 8
        xd, dd = dc.pack(x, xp, 0).to(dev), dc.pack(dz, dp, 0).to(dev)
        wsz = lib.rpc_dense_wgrad_workspace_size_f32(fmap, _ffi.int_arr(R), ci, co)
        assert wsz > 0 and wsz % (4 * ref.numel()) == 0
        ws = torch.full((wsz + 256,), 0xA5, dtype=torch.uint8, device=dev)
        # declined before any launch: a workspace one byte short
        dW = torch.full(ref.shape, float("nan"), device=dev)
        assert _wgrad(lib, fmap, kind, xd, xp, ci, dd, dp, co, R, S, O, dW, ws, wsz - 1) == dc.RPC_ERR_WORKSPACE
        torch.cuda.synchronize()
        assert torch.isnan(dW).all() and (ws == 0xA5).all(), what
        outs = []
        for _ in range(2):
            dW = torch.full(ref.shape, float("nan"), device=dev)
            _ffi.check(_wgrad(lib, fmap, kind, xd, xp, ci, dd, dp, co, R, S, O, dW, ws, wsz), what)
            torch.cuda.synchronize()
            outs.append(dW)
        assert (ws[wsz:] == 0xA5).all(), what                    # the stated workspace size is honoured
        got = outs[0].cpu().double()
        assert torch.isfinite(got).all(), what
        within(got, ref, (nt + 8) * U * mag, what, entry, WORST)
        assert torch.equal(raw(outs[0]), raw(outs[1])), what
    if img == (2, 48, 40) and fmap in (dc.S1, dc.S2):            # the case of more than one 32-row sub-tile per chunk
        chunks = lib.rpc_dense_wgrad_workspace_size_f32(fmap, _ffi.int_arr(R), 64, 64) // (4 * 9 * 64 * 64)
        assert dc.npix(R) > 32 * chunks


def test_wgrad_f32_guards_and_empty_image():
    lib = _ffi.load()
    dev = _dev()
    img, none = (1, 4, 4), (0, 4, 4)
    x = torch.zeros((16, 64), device=dev)
    dW = torch.full((9 * 64 * 64,), float("nan"), device=dev)
    wsz = lib.rpc_dense_wgrad_workspace_size_f32(dc.S1, _ffi.int_arr(img), 64, 64)
    ws = _ffi.workspace(wsz, dev)

    def wgrad(fmap=dc.S1, kind=0, xp=64, ci=64, dp=64, co=64, R=img):
        return _wgrad(lib, fmap, kind, x, xp, ci, x, dp, co, R, R, R, dW, ws, wsz)

    assert wgrad(fmap=dc.D2) == dc.RPC_ERR_ARG and wgrad(fmap=dc.G2) == dc.RPC_ERR_ARG
    assert wgrad(fmap=-1) == dc.RPC_ERR_ARG and wgrad(fmap=6) == dc.RPC_ERR_ARG
    assert wgrad(ci=32) == dc.RPC_ERR_ARG and wgrad(co=96) == dc.RPC_ERR_ARG
    assert wgrad(xp=66) == dc.RPC_ERR_ARG and wgrad(dp=70) == dc.RPC_ERR_ARG and wgrad(kind=2) == dc.RPC_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(dW).all()
    assert wgrad(R=none) == 0                                    # no rows: dW = 0
    torch.cuda.synchronize()
    assert (dW == 0).all()


# ------------------------------------------------------------------ rpc_dense_wprep_batch_f32
def _wprep_descs(dev, dtype, fill):
    """16 descriptors: WPREP_DESCS with both operands, WPREP_HALVES with one operand each way"""
    GUARD = 64
    items = [(d, True, True) for d in dc.WPREP_DESCS] + [(d, i % 2 == 0, i % 2 == 1)
                                                          for i, d in enumerate(dc.WPREP_HALVES)]
    descs, keep, wants = [], [], []
    for i, ((kind, ci, co, taps, flip, co_src), has_f, has_d) in enumerate(items):
        W = torch.randn(dc.wprep_source_shape(kind, ci, co, taps, co_src), generator=gen("wprep", i)) * 0.1
        if dtype == torch.bfloat16:
            W.view(-1)[::7] = dc.bf16_ties(W.view(-1)[::7].numel(), gen("ties", i))
        Wd = W.to(dev)
        n = taps * ci * co
        wf = torch.full((n + GUARD,), fill, dtype=dtype, device=dev) if has_f else None
        wdg = torch.full((n + GUARD,), fill, dtype=dtype, device=dev) if has_d else None
        descs.append(_ffi.RpcDenseWprep(Wd.data_ptr(), wf.data_ptr() if has_f else None,
                                        wdg.data_ptr() if has_d else None, kind, ci, co, taps, flip, co_src))
        keep.append((Wd, wf, wdg))
        wants.append((n, dc.wprep_ref(W, kind, co, flip)))
    return descs, keep, wants


def check_wprep_batch(entry, dtype):
    dev = _dev()
    descs, keep, wants = _wprep_descs(dev, dtype, 7.0)
    assert len(descs) == 16
    arr = (_ffi.RpcDenseWprep * 16)(*descs)
    _ffi.check(entry(arr, 16, _ffi.stream_of(keep[0][0])), "wprep_batch")
    torch.cuda.synchronize()
    for i, ((Wd, wf, wdg), (n, (rf, rd))) in enumerate(zip(keep, wants)):
        for got, want in ((wf, rf), (wdg, rd)):
            if got is not None:
                assert torch.equal(raw(got[:n]), raw(want.to(dtype).flatten())), (i, descs[i].kind)
                assert (got[n:] == 7.0).all(), i
        co_src, co = descs[i].co_src, descs[i].co
        if co_src and wf is not None:
            assert (wf[:n].view(descs[i].taps, co, -1)[:, co_src:] == 0).all()       # padded rows exactly zero
    # declined: 17 descriptors, and more source rows than outputs
    arr17 = (_ffi.RpcDenseWprep * 17)(*(descs + descs[:1]))
    assert entry(arr17, 17, _ffi.stream_of(keep[0][0])) == dc.RPC_ERR_ARG
    d = descs[8]
    bad = (_ffi.RpcDenseWprep * 1)(_ffi.RpcDenseWprep(d.W, d.w_fwd, d.w_dgrad, d.kind, d.ci, d.co, d.taps, d.flip,
                                                      d.co + 1))
    assert entry(bad, 1, _ffi.stream_of(keep[0][0])) == dc.RPC_ERR_ARG


def test_wprep_batch_f32_bit_exact():
    check_wprep_batch(_ffi.load().rpc_dense_wprep_batch_f32, torch.float32)


# ------------------------------------------------------------------ the fp32 BatchNorm passes
@pytest.mark.parametrize("C,M", dc.bn_shapes())
def test_bn_apply_f32(C, M):
    bp.check_bn_apply(_ffi.load(), F32, C, M, WORST)


@pytest.mark.parametrize("C,M", dc.bn_shapes())
def test_bnbwd_stats_f32(C, M):
    """the totals as for bf16 images, and every double partial row against the rows its block sums: the block of
    row m is (m // RL) % blocks with RL = 256 // (C / 8) row lanes (k_bnbwd_stats)"""
    r = bp.check_bnbwd_stats(_ffi.load(), F32, C, M, WORST)
    if r is None:
        return
    rows, dm, dmx = r
    nb, RL = rows.shape[0], 256 // (C // 8)
    blk = (torch.arange(M) // RL) % nb
    for k, term in enumerate((dm, dmx)):
        s = torch.zeros((nb, C), dtype=torch.float64).index_add_(0, blk, term)
        a = torch.zeros((nb, C), dtype=torch.float64).index_add_(0, blk, term.abs())
        within(rows[:, k * C:(k + 1) * C], s, (M + 8) * 2.0 ** -53 * a, f"bnbwd_stats_f32 rows C {C} M {M} [{k}]",
               "rpc_dense_bnbwd_stats_f32 rows (2^-53)", WORST)


@pytest.mark.parametrize("C,M", dc.bn_shapes())
def test_bnbwd_apply_f32(C, M):
    bp.check_bnbwd_apply(_ffi.load(), F32, C, M, WORST)


def test_bn_pass_argument_guards_f32():
    bp.check_bn_guards(_ffi.load(), F32)


@pytest.mark.parametrize("C,M", [(8, 7), (64, 257), (384, 4099), (2048, 255)])
def test_bnbwd_chain_f32(C, M):
    """stats -> rpc_bn_finalize(mode 1 | RPC_BN_PART_F64) -> apply, all through the ABI"""
    lib = _ffi.load()
    dev = _dev()
    g, bn, z, dh = bp.stats_case(F32, C, M, "chain")
    gamma = bn[:C] / bn[3 * C:]                                  # scale = gamma * invstd
    pitch, off = 2 * C + 8, C + 8
    dhd, zd, bd = dc.pack(dh, pitch, off, SPARE).to(dev), z.to(dev), bn.to(dev)
    gd, betad = gamma.to(dev), bn[C:2 * C].contiguous().to(dev)
    nb = lib.rpc_dense_bnbwd_blocks(M)
    part = torch.full((nb + 1, 2 * C), float("nan"), dtype=torch.float64, device=dev)
    st = _ffi.stream_of(zd)
    _ffi.check(lib.rpc_dense_bnbwd_stats_f32(_ffi.ptr(dhd), pitch, off, _ffi.ptr(zd), M, C, _ffi.ptr(bd),
                                             _ffi.ptr(part), st), "stats")
    bnb = torch.full((5 * C,), float("nan"), device=dev)
    dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
    _ffi.check(lib.rpc_bn_finalize(_ffi.ptr(part), nb, C, M, 1 | 4, _ffi.ptr(gd), _ffi.ptr(betad), 0.0, 0.0, None,
                                   None, _ffi.ptr(bd), _ffi.ptr(bnb), _ffi.ptr(dgamma), _ffi.ptr(dbeta), None, st),
               "rpc_bn_finalize")
    dz = dc.sentinel_buffer(M + SPARE, C, torch.float32).to(dev)
    _ffi.check(lib.rpc_dense_bnbwd_apply_f32(_ffi.ptr(dhd), pitch, off, _ffi.ptr(zd), M, C, _ffi.ptr(bd),
                                             _ffi.ptr(bnb), _ffi.ptr(dz), st), "apply")
    torch.cuda.synchronize()
    assert torch.isfinite(bnb).all() and dc.outside_unchanged(dz, M, C, 0)
    ref, mag = dc.bnbwd_apply_ref(dh, z, bn, bnb.cpu())
    within(dz[:M].cpu().double(), ref, 8 * U * mag, f"chain C {C} M {M}", "bnbwd chain f32", WORST)
    assert torch.equal(bnb[3 * C:].cpu(), bn[2 * C:])            # mean, invstd: the forward vector's, bit for bit
