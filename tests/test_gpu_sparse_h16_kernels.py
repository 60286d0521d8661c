"""The 16-bit sparse GEMM family in isolation through the C ABI: k_gemm_bf16 in its 11 tile shapes, its forward,
data-gradient, plain and eval-mode epilogues and both operand formats (rpc_spconv_gemm_h16, rpc_spconv_gemm_h16_infer,
rpc_spconv_gemm_bf16 / _n), the weight-tile prep (rpc_spconv_prep_weight_bf16 / _batch), the fp16 saturation of the
tile and row producers, and rpc_spconv_wgrad_bf16, element by element against the float64 references of
tests/_sparse_cases.py.

Operands. Source rows and weights are drawn on the 16-bit grid and the references read the same values back: the
tile prep rounds nothing and every product of two operands is exact in fp32, so only the fp32 accumulation is left.

Bounds. u = 2^-24, S = sum |a| |w| over the terms of an output element. An fp32 sum of n exact products in any
order lies within n * u * S of the exact one; every stored element of the GEMM is held to (K * kg + 8) * u * S, every
weight-gradient element to (n_k + 8) * u * S with n_k the number of rows that use offset k. This assumes that the
MFMA accumulates in fp32; it is derived, not measured. The eval-mode epilogue adds the accumulator's bound times
|scale| and 4 u (|acc * scale| + |shift| + |res|) for its fused multiply-add and its residual add. The BatchNorm
partial rows are compared with the column sums of the rows the kernel stored, within 72 u of their magnitudes (the
fp32 module's _check_part). The 16-bit rows of the eval-mode epilogue must be the stored fp32 rows rounded to nearest
even, bit for bit. ReLU masks of the data gradient are decided at least 1e-3 from zero and demanded exactly.

Measured on the MI355X (the module prints them when it ends; 459 tests in 9 s): worst err / tol per entry
    rpc_spconv_gemm_h16 epilogue 0   bf16 0.021   fp16 0.025   partial rows 0.040 / 0.041
    rpc_spconv_gemm_h16 epilogue 1   0.021   partial rows 0.050
    rpc_spconv_gemm_h16 epilogue 2   0.024
    rpc_spconv_gemm_h16_infer        bf16 0.25   fp16 0.25 (rows without a neighbour: one rounding of shift + res
                                     against the 4 u allowed)
    rpc_spconv_wgrad_bf16            0.040
No case misses its bound, so no step is added to it. Mutants of k_gemm_bf16 that stay in bounds, one run of this
module each: the offset order ignored fails the epilogue 1 and 2 tests (196); the last listed offset dropped fails
the epilogue 0, 1, 2 and eval-mode tests (392); the residual add omitted fails the eval-mode tests (98); one wave
left out of a partial row fails the epilogue 0 and 1 tests (196); the ReLU mask switched off fails the epilogue 1
tests (98); every wave skipping offsets by wave 0's mask fails all four GEMM tests (302 of 420); ones in the padding columns of the eval-mode rows fail the eval-mode tests of (24, 20), the one pair
with such columns (7). The first five were run before (24, 20) was added, on 98 cases per test.
"""
import zlib

import pytest
import torch

from robustpointclouds_amd import _ffi
from tests import _sparse_cases as sc

pytestmark = pytest.mark.gpu

U = sc.U
# (kg, ng): every compiled tile shape (round32(kg), round16(ng) / 16), then ragged widths; (24, 20) is the one whose
# output rows have padding columns (round8(ng) > ng)
PAIRS = [(16, 16), (16, 32), (32, 64), (32, 128), (64, 16), (64, 32), (64, 64), (64, 128), (128, 32), (128, 64),
         (128, 128), (20, 24), (40, 56), (100, 120), (24, 20)]
N_SRC = 300                               # source rows: more and fewer than n_out
ROWS = [1, 63, 64, 65, 129, 257, 2085]    # 2085: 17 blocks of 128 rows or 9 of 256, 33 partial rows
KS = [27, 3]
SPARE = 70                                # rows allocated beyond n_out, NaN-filled: nothing may write them
WG_PAIRS = [(16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128)]
WG_ROWS = [1, 255, 257, 513, 2049]
RPC_ERR_ARG, RPC_ERR_UNSUPPORTED = 1, 3
WORST = {}                                # entry -> worst err / tol seen


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"\nworst err/tol  {k:34s} {WORST[k]:.4f}", end="")
    print()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _within(got, ref, tol, what, entry):
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    fin = ratio[torch.isfinite(ratio)]
    if fin.numel():
        WORST[entry] = max(WORST.get(entry, 0.0), float(fin.max()))
    bad = ~(err <= tol)                    # a NaN counts as bad
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), float(ratio[bad].max()))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _check_part(part, nb, v, w, what, entry):
    """partial rows [nb, 2C] = per-64-row column sums of the stored rows v and of v * w, in float64 within 72 u of
    their magnitudes (64 additions, the product, and the two roundings of an xhat formed in fp32); the row after
    them is nobody's"""
    C = v.shape[1]
    assert part.shape[0] == nb + 1 and torch.isnan(part[nb]).all(), what
    p = part[:nb].cpu().double()
    s1, a1 = sc.tile_sums(v)
    s2, a2 = sc.tile_sums(v * w)
    _within(p[:, :C], s1, 72 * U * a1, what + " part[0]", entry + " part")
    _within(p[:, C:], s2, 72 * U * a2, what + " part[1]", entry + " part")


def _tiles(lib, Wd, dgrad, fmt):
    """weight tiles of W [K, ci, co] on the device through the ABI: the single-layer entry (bf16) or the batch"""
    K, ci, co = Wd.shape
    bt = torch.full((lib.rpc_spconv_bf16_weight_elems(K, ci, co, dgrad),), 7.0, dtype=sc.H16[fmt], device=Wd.device)
    st = _ffi.stream_of(Wd)
    if fmt == 0:
        _ffi.check(lib.rpc_spconv_prep_weight_bf16(_ffi.ptr(Wd), K, ci, co, dgrad, _ffi.ptr(bt), st), "prep_weight")
    else:
        desc = (_ffi.RpcSpconvWprep * 1)(_ffi.RpcSpconvWprep(Wd.data_ptr(), bt.data_ptr(), K, ci, co, dgrad, fmt))
        _ffi.check(lib.rpc_spconv_prep_weight_bf16_batch(desc, 1, st), "prep_weight_batch")
    torch.cuda.synchronize()
    return bt


def _gemm(lib, ad, fmt, kg, md, K, rev, n_out, bt, ng, epi, pz=None, pbn=None, with_part=False):
    dev = ad.device
    out = _nan((n_out + SPARE, ng), dev)
    nb = lib.rpc_spconv_gemm_blocks(n_out)
    assert nb == (n_out + 63) // 64
    part = _nan((nb + 1, 2 * ng), dev) if with_part else None
    _ffi.check(lib.rpc_spconv_gemm_h16(_ffi.ptr(ad), fmt, ad.shape[0], kg, _ffi.ptr(md), K, rev, n_out, _ffi.ptr(bt),
                                       ng, _ffi.ptr(out), _ffi.ptr(pz), _ffi.ptr(pbn), _ffi.ptr(part), epi,
                                       _ffi.stream_of(out)), "rpc_spconv_gemm_h16")
    torch.cuda.synchronize()
    return out, part


def _stored(out, n_out, what):
    assert torch.isnan(out[n_out:]).all(), what
    if n_out > 127:
        assert (out[64:128] == 0).all(), what                   # a 64-row tile without any neighbour
    return out[:n_out].cpu().double()


# ------------------------------------------------------------------ epilogue 0: z and BatchNorm partial rows
@pytest.mark.parametrize("n_out", ROWS)
@pytest.mark.parametrize("kg,ng", PAIRS)
def test_forward_epilogue_matches_fp64(kg, ng, n_out):
    lib = _ffi.load()
    dev = torch.device("cuda")
    nb = (n_out + 63) // 64
    for K in KS:
        mp = sc.random_map(n_out, N_SRC, K, seed=kg * 131 + ng + n_out + K)
        md = mp.to(dev)
        for fmt in (0, 1):
            what = f"epi 0 ({kg},{ng}) n_out {n_out} K {K} fmt {fmt}"
            g = _gen("fwd", kg, ng, n_out, K, fmt)
            a = sc.h16_rows(N_SRC, kg, g, fmt)
            W = sc.h16_weights(K, kg, ng, g, fmt)
            ref, S = sc.gather_gemm_ref(a, mp, 0, W)
            ad = a.to(dev)
            bt = _tiles(lib, W.to(dev), 0, fmt)
            out, part = _gemm(lib, ad, fmt, kg, md, K, 0, n_out, bt, ng, 0, with_part=True)
            got = _stored(out, n_out, what)
            _within(got, ref, (K * kg + 8) * U * S, what, f"gemm_h16 epi 0 fmt {fmt}")
            assert (ref[0] != 0).all()                           # row 0 always has a neighbour
            _check_part(part, nb, got, got, what, f"gemm_h16 epi 0 fmt {fmt}")
            out2, _ = _gemm(lib, ad, fmt, kg, md, K, 0, n_out, bt, ng, 0)                 # part = NULL
            assert torch.equal(out2[:n_out], out[:n_out]) and torch.isnan(out2[n_out:]).all(), what
            out3, part3 = _gemm(lib, ad, fmt, kg, md, K, 0, n_out, bt, ng, 0, with_part=True)
            assert torch.equal(out3[:n_out], out[:n_out]) and torch.equal(part3[:nb], part[:nb]), what


# ------------------------------------------------------------------ epilogues 2 and 1: the data gradient's GEMM
def _dgrad_case(lib, dev, tag, kg, ng, n_out, K):
    """bf16 rows of width kg = co through the data-gradient tiles of W [K, ci = ng, co = kg]: B_k = W[k]^T"""
    g = _gen(tag, kg, ng, n_out, K)
    a = sc.h16_rows(N_SRC, kg, g, 0)
    W = sc.h16_weights(K, ng, kg, g, 0)
    mp = sc.random_map(n_out, N_SRC, K, seed=kg * 137 + ng + n_out + K)
    if mp[0, K - 1] == mp[0, 0]:                                 # a single row can draw its first neighbour again
        mp[0, K - 1] = 0
    assert not torch.equal(mp[:1], mp[:1].flip(1))               # not symmetric under k -> K-1-k, from row 0 on
    return g, a, W, mp, a.to(dev), mp.to(dev), _tiles(lib, W.to(dev), 1, 0)


@pytest.mark.parametrize("n_out", ROWS)
@pytest.mark.parametrize("kg,ng", PAIRS)
def test_plain_epilogue_rev_matches_fp64(kg, ng, n_out):
    lib = _ffi.load()
    dev = torch.device("cuda")
    for K in KS:
        g, a, W, mp, ad, md, bt = _dgrad_case(lib, dev, "plain", kg, ng, n_out, K)
        refs = []
        for rev in (0, 1):
            what = f"epi 2 ({kg},{ng}) n_out {n_out} K {K} rev {rev}"
            ref, S = sc.gather_gemm_ref(a, mp, rev, W.transpose(1, 2))
            out, _ = _gemm(lib, ad, 0, kg, md, K, rev, n_out, bt, ng, 2)
            _within(_stored(out, n_out, what), ref, (K * kg + 8) * U * S, what, "gemm_h16 epi 2")
            refs.append(ref)
        assert not torch.equal(refs[0], refs[1])                 # the two orders are different sums


@pytest.mark.parametrize("n_out", ROWS)
@pytest.mark.parametrize("kg,ng", PAIRS)
def test_dgrad_epilogue_mask_and_partials_match_fp64(kg, ng, n_out):
    lib = _ffi.load()
    dev = torch.device("cuda")
    nb = (n_out + 63) // 64
    for K in KS:
        g, a, W, mp, ad, md, bt = _dgrad_case(lib, dev, "dgrad", kg, ng, n_out, K)
        prev_bn = sc.bn_vec(ng, g)
        prev_z = sc.decisive_z(n_out, prev_bn, g)
        keep = sc.relu_mask_ref(prev_z, prev_bn)
        sc_, be_, mu_, is_ = prev_bn.double().view(4, ng)
        xh = (prev_z.double() - mu_) * is_
        pzd, pbd = prev_z.to(dev), prev_bn.to(dev)
        for rev in (0, 1):
            what = f"epi 1 ({kg},{ng}) n_out {n_out} K {K} rev {rev}"
            ref, S = sc.gather_gemm_ref(a, mp, rev, W.transpose(1, 2))
            out, part = _gemm(lib, ad, 0, kg, md, K, rev, n_out, bt, ng, 1, pzd, pbd, with_part=True)
            got = _stored(out, n_out, what)
            _within(got, ref * keep, (K * kg + 8) * U * S * keep, what, "gemm_h16 epi 1")
            assert (got[~keep] == 0).all() and (got[keep] != 0).any(), what               # the exact mask
            _check_part(part, nb, got, xh, what, "gemm_h16 epi 1")


# ------------------------------------------------------------------ the eval-mode epilogue
@pytest.mark.parametrize("n_out", ROWS)
@pytest.mark.parametrize("kg,ng", PAIRS)
def test_infer_epilogue_matches_fp64(kg, ng, n_out):
    lib = _ffi.load()
    dev = torch.device("cuda")
    op = sc.r8(ng)
    for K in KS:
        mp = sc.random_map(n_out, N_SRC, K, seed=kg * 139 + ng + n_out + K)
        md = mp.to(dev)
        for fmt in (0, 1):
            g = _gen("infer", kg, ng, n_out, K, fmt)
            a = sc.h16_rows(N_SRC, kg, g, fmt)
            W = sc.h16_weights(K, kg, ng, g, fmt)
            fold = sc.bn_vec(ng, g)[:2 * ng].contiguous()          # scale of either sign, shift
            res = torch.randn((n_out, ng), generator=g)
            acc, S = sc.gather_gemm_ref(a, mp, 0, W)
            ad, fd, rd = a.to(dev), fold.to(dev), res.to(dev)
            bt = _tiles(lib, W.to(dev), 0, fmt)
            st = _ffi.stream_of(ad)
            for with_res in (False, True):
                what = f"infer ({kg},{ng}) n_out {n_out} K {K} fmt {fmt} res {with_res}"
                y, M = sc.infer_ref(acc, fold, res if with_res else None)
                tol = (K * kg + 8) * U * S * fold[:ng].double().abs() + 4 * U * M
                rows = []
                for with_f32 in (True, False):
                    oh = torch.full((n_out + SPARE, op), 7.0, dtype=sc.H16[fmt], device=dev)
                    of = _nan((n_out + SPARE, ng), dev) if with_f32 else None
                    _ffi.check(lib.rpc_spconv_gemm_h16_infer(_ffi.ptr(ad), fmt, N_SRC, kg, _ffi.ptr(md), K, n_out,
                                                             _ffi.ptr(bt), ng, _ffi.ptr(fd),
                                                             _ffi.ptr(rd) if with_res else None, _ffi.ptr(oh),
                                                             _ffi.ptr(of), st), "rpc_spconv_gemm_h16_infer")
                    torch.cuda.synchronize()
                    assert (oh[n_out:] == 7.0).all(), what       # rows past n_out keep their marker
                    assert (oh[:n_out, ng:] == 0).all(), what    # padding columns
                    rows.append(oh[:n_out])
                    if with_f32:
                        assert torch.isnan(of[n_out:]).all(), what
                        _within(of[:n_out].cpu().double(), y, tol, what, f"gemm_h16_infer fmt {fmt}")
                        # the operand rows: the stored fp32 rows rounded to nearest even, bit for bit
                        assert torch.equal(_bits(oh[:n_out, :ng]), _bits(of[:n_out].cpu().to(sc.H16[fmt]))), what
                assert torch.equal(_bits(rows[0]), _bits(rows[1])), what
                if n_out >= 63:
                    assert (y == 0).any() and (y > 0).any()      # the ReLU both clips and passes


# ------------------------------------------------------------------ the older entry points
def test_legacy_entries_equal_gemm_h16():
    """rpc_spconv_gemm_bf16 (source bounded by n_out rows) and rpc_spconv_gemm_bf16_n are rpc_spconv_gemm_h16 with
    fmt 0: the same bits."""
    lib = _ffi.load()
    dev = torch.device("cuda")
    # rpc_spconv_gemm_bf16: forward epilogue with partial rows, (64, 64)
    kg, ng, n_out, K = 64, 64, 257, 27
    g = _gen("legacy", 0)
    a, W = sc.h16_rows(N_SRC, kg, g, 0), sc.h16_weights(K, kg, ng, g, 0)
    ad, md = a.to(dev), sc.random_map(n_out, N_SRC, K, seed=1).to(dev)
    bt = _tiles(lib, W.to(dev), 0, 0)
    want, wpart = _gemm(lib, ad, 0, kg, md, K, 0, n_out, bt, ng, 0, with_part=True)
    out, part = _nan((n_out + SPARE, ng), dev), _nan(tuple(wpart.shape), dev)
    _ffi.check(lib.rpc_spconv_gemm_bf16(_ffi.ptr(ad), kg, _ffi.ptr(md), K, 0, n_out, _ffi.ptr(bt), ng, _ffi.ptr(out),
                                        None, None, _ffi.ptr(part), 0, _ffi.stream_of(out)), "rpc_spconv_gemm_bf16")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))                     # NaN spare rows included
    assert torch.equal(part[:-1], wpart[:-1]) and torch.isnan(part[-1]).all()
    # rpc_spconv_gemm_bf16_n: data-gradient epilogue, reversed offsets, ragged (40, 56)
    kg, ng, n_out = 40, 56, 129
    g = _gen("legacy", 1)
    a, W = sc.h16_rows(N_SRC, kg, g, 0), sc.h16_weights(K, ng, kg, g, 0)
    prev_bn = sc.bn_vec(ng, g)
    pzd, pbd = sc.decisive_z(n_out, prev_bn, g).to(dev), prev_bn.to(dev)
    ad, md = a.to(dev), sc.random_map(n_out, N_SRC, K, seed=2).to(dev)
    bt = _tiles(lib, W.to(dev), 1, 0)
    want, wpart = _gemm(lib, ad, 0, kg, md, K, 1, n_out, bt, ng, 1, pzd, pbd, with_part=True)
    out, part = _nan((n_out + SPARE, ng), dev), _nan(tuple(wpart.shape), dev)
    _ffi.check(lib.rpc_spconv_gemm_bf16_n(_ffi.ptr(ad), N_SRC, kg, _ffi.ptr(md), K, 1, n_out, _ffi.ptr(bt), ng,
                                          _ffi.ptr(out), _ffi.ptr(pzd), _ffi.ptr(pbd), _ffi.ptr(part), 1,
                                          _ffi.stream_of(out)), "rpc_spconv_gemm_bf16_n")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    assert torch.equal(part[:-1], wpart[:-1]) and torch.isnan(part[-1]).all()
    assert not torch.isnan(want[:n_out]).any() and (want[:n_out] != 0).any()


# ------------------------------------------------------------------ argument guards: declined before any launch
def test_gemm_argument_guards():
    lib = _ffi.load()
    dev = torch.device("cuda")
    K, n_out = 27, 100
    a = torch.zeros((N_SRC, 136), dtype=torch.bfloat16, device=dev)
    a16 = torch.zeros((N_SRC, 136), dtype=torch.float16, device=dev)
    bt = torch.zeros((K * 144 * 160,), dtype=torch.bfloat16, device=dev)
    md = sc.random_map(n_out, N_SRC, K, seed=9).to(dev)
    out = _nan((n_out, 144), dev)
    part = _nan((2, 2 * 144), dev)
    pz, pbn = torch.zeros((n_out, 144), device=dev), torch.ones((4 * 144,), device=dev)
    oh = torch.full((n_out, 144), 7.0, dtype=torch.bfloat16, device=dev)
    st = _ffi.stream_of(out)
    P = _ffi.ptr

    def gemm_n(n_src, kg, ng, n):
        return lib.rpc_spconv_gemm_bf16_n(P(a), n_src, kg, P(md), K, 0, n, P(bt), ng, P(out), None, None, P(part), 0, st)

    # the 2 GiB source table (32-bit buffer offsets): n_src * round8(kg) * 2 bytes
    assert gemm_n(2 ** 23, 128, 128, 0) == RPC_ERR_UNSUPPORTED
    assert gemm_n(2 ** 23 - 1, 128, 128, 0) == 0
    # widths without a compiled tile shape
    for kg, ng in [(128, 16), (40, 72), (130, 64), (64, 144)]:
        assert gemm_n(N_SRC, kg, ng, n_out) == RPC_ERR_UNSUPPORTED, (kg, ng)
        for epi in (0, 1, 2):
            assert lib.rpc_spconv_gemm_h16(P(a), 0, N_SRC, kg, P(md), K, 0, n_out, P(bt), ng, P(out), P(pz), P(pbn),
                                           P(part), epi, st) == RPC_ERR_UNSUPPORTED, (kg, ng, epi)
        for fmt, rows in ((0, a), (1, a16)):
            assert lib.rpc_spconv_gemm_h16_infer(P(rows), fmt, N_SRC, kg, P(md), K, n_out, P(bt), ng, P(pbn), None,
                                                 P(oh), P(out), st) == RPC_ERR_UNSUPPORTED, (kg, ng, fmt)
    # fp16 operands: the forward and the eval-mode epilogues only
    for epi in (1, 2):
        assert lib.rpc_spconv_gemm_h16(P(a16), 1, N_SRC, 64, P(md), K, 0, n_out, P(bt), 64, P(out), P(pz), P(pbn),
                                       P(part), epi, st) == RPC_ERR_UNSUPPORTED
    # the eval-mode entry's own checks
    infer = lambda fmt, fold, o16: lib.rpc_spconv_gemm_h16_infer(P(a), fmt, N_SRC, 64, P(md), K, n_out, P(bt), 64, fold,
                                                                 None, o16, P(out), st)
    assert infer(2, P(pbn), P(oh)) == RPC_ERR_ARG
    assert infer(0, None, P(oh)) == RPC_ERR_ARG
    assert infer(0, P(pbn), None) == RPC_ERR_ARG
    # no rows: success, nothing written
    assert lib.rpc_spconv_gemm_h16(P(a), 0, N_SRC, 64, P(md), K, 0, 0, P(bt), 64, P(out), None, None, P(part), 0,
                                   st) == 0
    assert lib.rpc_spconv_gemm_h16_infer(P(a), 0, N_SRC, 64, P(md), K, 0, P(bt), 64, P(pbn), None, P(oh), P(out),
                                         st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(part).all() and (oh == 7.0).all()


# ------------------------------------------------------------------ weight tiles
TILE_DESCS = [(27, 16, 32), (3, 20, 24), (27, 40, 56), (27, 64, 128), (1, 100, 120)]
GUARD = 64                                # elements after each tile buffer that the prep must leave alone


def _same_tiles(got, want):
    """bit for bit, except that a NaN need only be a NaN"""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(_bits(got.masked_fill(gn, 0)), _bits(want.masked_fill(wn, 0)))


def test_weight_tiles_bit_exact():
    """off-grid fp32 weights: the tiles are torch's rounding of W in the header's layout, padding zero; the batch
    launch writes what the single-layer launch writes"""
    lib = _ffi.load()
    dev = torch.device("cuda")
    Ws, single, descs, bufs, wants = [], {}, [], [], []
    for i, (K, ci, co) in enumerate(TILE_DESCS):
        W = torch.randn((K, ci, co), generator=_gen("tiles", i)) * 0.1
        Wd = W.to(dev)
        Ws.append(Wd)
        for dgrad in (0, 1):
            want = sc.weight_tiles_ref(W, dgrad, 0)
            n = lib.rpc_spconv_bf16_weight_elems(K, ci, co, dgrad)
            assert n == want.numel()
            bt = torch.full((n + GUARD,), 7.0, dtype=torch.bfloat16, device=dev)
            _ffi.check(lib.rpc_spconv_prep_weight_bf16(_ffi.ptr(Wd), K, ci, co, dgrad, _ffi.ptr(bt),
                                                       _ffi.stream_of(bt)), "prep_weight")
            torch.cuda.synchronize()
            assert torch.equal(_bits(bt[:n]), _bits(want.flatten())), (K, ci, co, dgrad)
            assert (bt[n:] == 7.0).all()
            single[(i, dgrad, 0)] = bt[:n]
        for dgrad, fmt in ((0, 0), (1, 0), (0, 1)):
            want = sc.weight_tiles_ref(W, dgrad, fmt)
            bt = torch.full((want.numel() + GUARD,), 7.0, dtype=sc.H16[fmt], device=dev)
            descs.append(_ffi.RpcSpconvWprep(Wd.data_ptr(), bt.data_ptr(), K, ci, co, dgrad, fmt))
            bufs.append(bt)
            wants.append(((i, dgrad, fmt), want))
    arr = (_ffi.RpcSpconvWprep * len(descs))(*descs)
    _ffi.check(lib.rpc_spconv_prep_weight_bf16_batch(arr, len(descs), _ffi.stream_of(bufs[0])), "prep_weight_batch")
    torch.cuda.synchronize()
    for bt, (key, want) in zip(bufs, wants):
        n = want.numel()
        assert torch.equal(_bits(bt[:n]), _bits(want.flatten())), key
        assert (bt[n:] == 7.0).all(), key
        if key[2] == 0:
            assert torch.equal(_bits(bt[:n]), _bits(single[key])), key


SPECIALS = [1e5, -7e4, 65504.0, 65519.0, 65520.0, -65520.0, 3.0e38, float("inf"), float("-inf"), float("nan")]


def test_fp16_saturation_in_tiles_and_rows():
    """a finite weight or activation beyond +-65504 becomes +-65504 in fp16, inf / NaN pass through; the bf16 copy of
    the rows is not clamped"""
    lib = _ffi.load()
    dev = torch.device("cuda")
    sp = torch.tensor(SPECIALS)
    K, ci, co = 3, 20, 24
    W = torch.randn((K, ci, co), generator=_gen("sat")) * 0.1
    W.view(-1)[torch.arange(len(SPECIALS)) * 97 + 5] = sp
    want = sc.weight_tiles_ref(W, 0, 1)
    got = _tiles(lib, W.to(dev), 0, 1).cpu().view(want.shape)
    assert _same_tiles(got, want)
    f = got.float()
    assert (f == 65504.0).sum() == 5 and (f == -65504.0).sum() == 2 and torch.isinf(f).sum() == 2
    assert torch.isnan(f).sum() == 1
    for c in (16, 20):                                           # the 8-channel and the scalar producer
        n, cp = 70, sc.r8(c)
        z = torch.randn((n, c), generator=_gen("satrows", c)) * 2
        z.view(-1)[torch.arange(len(SPECIALS)) * 53 + 3] = sp
        z.view(-1)[-len(SPECIALS):] = -sp                        # the last row, the other signs
        zd = z.to(dev)
        h = torch.full((n, cp), 7.0, dtype=torch.float16, device=dev)
        hb = torch.full((n, cp), 7.0, dtype=torch.bfloat16, device=dev)
        _ffi.check(lib.rpc_to_h16_rows(_ffi.ptr(zd), None, n, c, 0, 1, _ffi.ptr(h), _ffi.ptr(hb), _ffi.stream_of(h)),
                   "rpc_to_h16_rows")
        torch.cuda.synchronize()
        assert _same_tiles(h[:, :c].cpu(), sc.to_h16(z, 1)), c
        assert _same_tiles(hb[:, :c].cpu(), z.to(torch.bfloat16)), c
        assert (h[:, c:] == 0).all() and (hb[:, c:] == 0).all()
        f = h[:, :c].float()
        assert (f.abs() == 65504.0).sum() == 14 and torch.isinf(f).sum() == 4 and torch.isnan(f).sum() == 2
        assert torch.isinf(hb[:, :c].float()).sum() == 4 and (hb[:, :c].float().abs() > 9e4).sum() >= 6


# ------------------------------------------------------------------ weight gradient, element by element
@pytest.mark.parametrize("n_out", WG_ROWS)
@pytest.mark.parametrize("ci,co", WG_PAIRS)
def test_wgrad_bf16_elementwise(ci, co, n_out):
    lib = _ffi.load()
    dev = torch.device("cuda")
    for K in KS:
        what = f"wgrad_bf16 ({ci},{co}) n_out {n_out} K {K}"
        g = _gen("wgrad", ci, co, n_out, K)
        h = sc.h16_rows(N_SRC, ci, g, 0)
        dz = sc.h16_rows(n_out, co, g, 0)
        nbr = sc.random_map(n_out, N_SRC, K, seed=ci * 149 + co + n_out + K)
        ref, S, nk = sc.gather_wgrad_ref(h, nbr, dz)
        hd, dd, nd = h.to(dev), dz.to(dev), nbr.to(dev)
        wsz = lib.rpc_spconv_wgrad_bf16_workspace_size(n_out, K, ci, co)
        ws = _ffi.workspace(wsz, dev)
        outs = []
        for _ in range(2):
            dW = _nan((K, ci, co), dev)
            _ffi.check(lib.rpc_spconv_wgrad_bf16(_ffi.ptr(hd), ci, _ffi.ptr(nd), K, n_out, _ffi.ptr(dd), co,
                                                 _ffi.ptr(dW), _ffi.ptr(ws), wsz, _ffi.stream_of(dW)), "wgrad_bf16")
            torch.cuda.synchronize()
            outs.append(dW)
        got = outs[0].cpu().double()
        assert torch.isfinite(got).all(), what
        _within(got, ref, (nk + 8).double().view(K, 1, 1) * U * S, what, "wgrad_bf16")
        assert nk[1] == 0 and (outs[0][1] == 0).all(), what       # the offset nobody uses
        if n_out > 63:
            assert nk[K - 1] == 1 and (ref[K - 1] != 0).all()     # the offset only row 63 uses: one term each
        assert torch.equal(outs[0], outs[1]), what
