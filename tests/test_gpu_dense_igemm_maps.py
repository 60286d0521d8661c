"""The bf16 dense engine's GEMMs entry by entry through the C ABI: rpc_dense_conv on every map (the implicit GEMM
k_igemm for S2, D2, P1, U2, G2 and each of the four stride-1 kernels forced by knob 0), rpc_dense_wgrad and
rpc_dense_wprep / _batch, element by element against the float64 references of tests/_dense_cases.py.

Operands are drawn on the bf16 grid, so every product is exact in fp32 and only the fp32 accumulation and the one
rounding of the output to bf16 are left. u = 2^-24, n = taps * cin, mag = sum |a| |w|.

Bounds, derived and not measured:
    conv      every stored element within 2^-8 (|ref| + e) + e of float64, e = (n + 8) u mag: an fp32 sum of n exact
              products in any order, then one round-to-nearest-even to bf16. With accumulate the base is added in
              fp32 before that rounding: ref and e grow by the base and by u (|acc| + |base|).
    partials  exactly rpc_dense_conv_part_rows rows are written (the next keeps its sentinel); the float64 column
              totals of both halves lie within (rows per tile + 8) u of the magnitudes of the stored values and of
              their squares: a tile's rows are summed in fp32 (rows - 1 additions; a bf16 value and its square are
              exact in fp32), which is _check_part's 72 = 64 + 8 of the sparse modules for a tile of TM = 128 rows
              (k_igemm), 256 (the 16 x 16 tiles of the stride-1 kernels) or 512 (k_conv3x3x's 16 x 32).
    wgrad     (n_t + 8) u mag, n_t = rows whose tap t lies inside the image (slabs summed in double, one rounding).
    wprep     torch's fp32 -> bf16 cast of a permutation, bit for bit, on values that include exact ties.

Measured on the MI355X (the module prints them when it ends; 67 tests in 4 s): worst err / tol per entry
    rpc_dense_conv   S2 0.95  D2 0.98  P1 0.99  U2 0.99  G2 0.98; partial rows 0.010 .. 0.021
    stride-1 kernels k_conv3x3 (64 and 32 channels per block), k_conv3x3w, k_conv3x3x, k_conv3x3y: 0.955 each (the
                     same bits on these cases); partial rows 0.005 .. 0.008
    rpc_dense_wgrad  S1 0.014  S2 0.013  P1 0.007  U2 0.008
The ratios near 1 are the rounding to bf16 itself and no missed term: half an ulp is 2^-8 of the lower end of a
binade, so an accumulator near a tie just above a power of two uses all of 2^-8 |ref|; the fp32 part alone is
what the weight gradient shows, which is not rounded to bf16 and stays below 0.02 of its bound.
No case misses its bound. No kernel bug was found.
Mutants that stay in bounds, one build and one run of this module each: k_igemm<M_U2> with the parity bits swapped in
out_row fails test_igemm_maps_match_fp64 on U2 (5 of 5 images); k_igemm adding the accumulate base after the
rounding to bf16 fails it on D2 and G2, the maps run with accumulate (12 of 12).
"""
import functools

import pytest
import torch

from robustpointclouds_amd import _ffi
from tests import _dense_cases as dc
from tests import test_gpu_dense_bn_passes as bp
from tests import test_gpu_dense_f32_kernels as f32t

pytestmark = pytest.mark.gpu

U = dc.U
SPARE = 3
WORST = {}
within, gen, raw, knob = bp.within, bp.gen, bp.raw, bp.knob
BF = torch.bfloat16
IG_MAPS = [dc.S2, dc.D2, dc.P1, dc.U2, dc.G2]
IG_CASES = [(m, i) for m in IG_MAPS for i in range(len(dc.conv_cases(m, dc.IMAGES_BF16)))]
# knob 0 (and knob 5 for the register-staged kernel) -> what rpc_dense_conv_s1_kernel must answer, rows per tile
S1_KERNELS = [((1, 1), 0, 256), ((1, 2), 0, 256), ((2, 0), 1, 256), ((3, 0), 2, 512), ((4, 0), 3, 256)]


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    bp.report(WORST)


def _dev():
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _case(fmap, R, S, O, cin, cout):
    """operands on the bf16 grid and their float64 reference, computed once and left unchanged"""
    g = gen("igemm", fmap, R, S, cin, cout)
    x = dc.bf16_grid(dc.npix(S), cin, gen=g)
    W = dc.bf16_grid(*dc.layer_weight_shape(fmap, cin, cout), gen=g, scale=0.1)
    base = dc.bf16_grid(dc.npix(O), cout, gen=g)
    ref, mag = dc.conv_ref(fmap, x, W, dc.KIND[fmap], R, S, O)
    return x, dc.gemm_weights(fmap, W), base, ref, mag


def _conv(lib, fmap, xd, sp, cin, wd, cout, out, op, ooff, accum, part, R, S, O):
    _ffi.check(lib.rpc_dense_conv(dc.ABI_MAP[fmap], _ffi.ptr(xd), sp, cin, _ffi.ptr(wd), cout, _ffi.ptr(out), op,
                                  ooff, accum, _ffi.ptr(part), _ffi.int_arr(R), _ffi.int_arr(S), _ffi.int_arr(O),
                                  _ffi.stream_of(out)), "rpc_dense_conv")
    torch.cuda.synchronize()


def _check_totals(part, nrows, tile, got, what, entry):
    assert part.shape[0] == nrows + 1 and torch.isnan(part[nrows]).all(), what
    assert torch.isfinite(part[:nrows]).all(), what
    Cc = got.shape[1]
    tot = part[:nrows].cpu().double().sum(0)
    within(tot[:Cc], got.sum(0), (tile + 8) * U * got.abs().sum(0), what + " part[0]", entry + " part", WORST)
    within(tot[Cc:], (got * got).sum(0), (tile + 8) * U * (got * got).sum(0), what + " part[1]", entry + " part",
           WORST)


def _run_ways(lib, fmap, R, S, O, cin, cout, ways, nrows, tile, entry, tag=""):
    """every way of one case: [(way, with_part)] -> {(way, with_part): raw bits of the stored image}"""
    dev = _dev()
    x, wt, base, ref, mag = _case(fmap, R, S, O, cin, cout)
    Mo, n = dc.npix(O), dc.TAPS[fmap] * cin
    wd = wt.to(dev)
    geo = {"dense": (cin, cout, 0, 0), "pitched": (cin + 16, 2 * cout + 8, cout + 8, 0),
           "accumulate": (cin, cout, 0, 1)}
    bits = {}
    for way, with_part in ways:
        sp, op, ooff, accum = geo[way]
        what = f"{entry}{tag} {R} <- {S} ({cin},{cout}) {way} part {with_part}"
        xd = dc.pack(x, sp, 0).to(dev)
        out = (dc.pack(base, op, ooff, SPARE) if accum else dc.sentinel_buffer(Mo + SPARE, op, BF)).to(dev)
        part = torch.full((nrows + 1, 2 * cout), float("nan"), device=dev) if with_part else None
        _conv(lib, fmap, xd, sp, cin, wd, cout, out, op, ooff, accum, part, R, S, O)
        assert dc.outside_unchanged(out, Mo, cout, ooff), what
        stored = dc.unpack(out, Mo, cout, ooff).cpu()
        got = stored.double()
        e = (n + 8) * U * mag
        r = ref
        if accum:
            r = ref + base.double()
            e = e + U * (ref.abs() + base.double().abs())
        within(got, r, 2.0 ** -8 * (r.abs() + e) + e, what, entry, WORST)
        if with_part:
            _check_totals(part, nrows, tile, got, what, entry)
        bits[(way, with_part)] = raw(stored)
    return bits


# ------------------------------------------------------------------ k_igemm: S2, D2, P1, U2, G2
@pytest.mark.parametrize("fmap,idx", IG_CASES)
def test_igemm_maps_match_fp64(fmap, idx):
    lib = _ffi.load()
    R, S, O = dc.conv_cases(fmap, dc.IMAGES_BF16)[idx]
    entry = "conv " + dc.MAP_NAMES[fmap]
    ways = [("dense", True), ("dense", False), ("pitched", True)]
    if fmap in (dc.D2, dc.G2):                                   # production accumulates data gradients
        ways += [("accumulate", True), ("accumulate", False)]
    for cin, cout in dc.CHANNELS_BF16:
        nrows = lib.rpc_dense_conv_part_rows(dc.ABI_MAP[fmap], cout, _ffi.int_arr(R))
        assert nrows == (dc.npix(R) + 127) // 128 * (4 if fmap == dc.U2 else 1)
        assert nrows == lib.rpc_dense_conv_blocks(dc.ABI_MAP[fmap], _ffi.int_arr(R))
        bits = _run_ways(lib, fmap, R, S, O, cin, cout, ways, nrows, 128, entry)
        if fmap != dc.D2:        # D2 without partial rows is the parity-split form: in bounds, not the same bits
            assert torch.equal(bits[("dense", True)], bits[("dense", False)]), (entry, R, cin, cout)
        if cout == 256:                                          # the flat grid order against the 2-D one
            with knob(lib, 2, 1):
                bits2 = _run_ways(lib, fmap, R, S, O, cin, cout, ways, nrows, 128, entry, " 2-D")
            for k in bits:
                assert torch.equal(bits[k], bits2[k]), (entry, R, cin, cout, k)


# ------------------------------------------------------------------ the stride-1 kernels
@pytest.mark.parametrize("img", dc.IMAGES_S1_BF16)
@pytest.mark.parametrize("knobs,kernel,tile", S1_KERNELS)
def test_s1_kernels_match_fp64(knobs, kernel, tile, img):
    lib = _ffi.load()
    ways = [("dense", True), ("dense", False), ("pitched", True), ("accumulate", True)]
    with knob(lib, 0, knobs[0]), knob(lib, 5, knobs[1]):
        for cin, cout in dc.CHANNELS_S1_BF16:
            assert lib.rpc_dense_conv_s1_kernel(dc.S1, cout, _ffi.int_arr(img)) == kernel
            nrows = lib.rpc_dense_conv_part_rows(dc.S1, cout, _ffi.int_arr(img))
            tw = 32 if tile == 512 else 16
            assert nrows == img[0] * ((img[1] + 15) // 16) * ((img[2] + tw - 1) // tw)
            entry = f"conv S1 knob0 {knobs[0]} knob5 {knobs[1]}"
            bits = _run_ways(lib, dc.S1, img, img, img, cin, cout, ways, nrows, tile, entry)
            assert torch.equal(bits[("dense", True)], bits[("dense", False)]), (entry, img, cin, cout)


# ------------------------------------------------------------------ rpc_dense_wgrad
@pytest.mark.parametrize("img", dc.WGRAD_IMAGES_BF16)
@pytest.mark.parametrize("fmap", [dc.S1, dc.S2, dc.P1, dc.U2])
def test_wgrad_bf16_matches_fp64(fmap, img):
    lib = _ffi.load()
    dev = _dev()
    R, S, O = dc.wgrad_geometry(fmap, img)
    kind = dc.KIND[fmap]
    entry = "wgrad " + dc.MAP_NAMES[fmap]
    with knob(lib, 1, 1):                                        # S1: the generic k_wgrad
        for ci, co in dc.WGRAD_CHANNELS:
            what = f"{entry} {R} ({ci},{co})"
            g = gen("wgrad", fmap, img, ci, co)
            x = dc.bf16_grid(dc.npix(S), ci, gen=g)
            dz = dc.bf16_grid(dc.npix(O), co, gen=g)
            ref, mag = dc.wgrad_ref(fmap, x, dz, kind, R, S, O)
            nt = dc.wgrad_bound_terms(fmap, kind, R, S, ref.shape)
            xp, dp = ci + 16, co + 8
            xd, dd = dc.pack(x, xp, 0).to(dev), dc.pack(dz, dp, 0).to(dev)
            wsz = lib.rpc_dense_wgrad_workspace_size(fmap, _ffi.int_arr(R), ci, co)
            ws = torch.full((wsz + 256,), 0xA5, dtype=torch.uint8, device=dev)
            outs = []
            for _ in range(2):
                dW = torch.full(ref.shape, float("nan"), device=dev)
                _ffi.check(lib.rpc_dense_wgrad(fmap, kind, _ffi.ptr(xd), xp, ci, _ffi.ptr(dd), dp, co, _ffi.int_arr(R),
                                               _ffi.int_arr(S), _ffi.int_arr(O), _ffi.ptr(dW), _ffi.ptr(ws), wsz,
                                               _ffi.stream_of(dW)), what)
                torch.cuda.synchronize()
                outs.append(dW)
            assert (ws[wsz:] == 0xA5).all(), what
            got = outs[0].cpu().double()
            assert torch.isfinite(got).all(), what
            within(got, ref, (nt + 8) * U * mag, what, entry, WORST)
            assert torch.equal(raw(outs[0]), raw(outs[1])), what


# ------------------------------------------------------------------ rpc_dense_wprep / _batch
def test_wprep_batch_bf16_bit_exact():
    f32t.check_wprep_batch(_ffi.load().rpc_dense_wprep_batch, BF)


def test_wprep_single_bf16_bit_exact():
    lib = _ffi.load()
    dev = _dev()
    for i, (kind, ci, co, taps, flip, co_src) in enumerate(dc.WPREP_DESCS):
        if co_src:
            continue                                             # the single-layer entry has no padded rows
        W = torch.randn(dc.wprep_source_shape(kind, ci, co, taps, 0), generator=gen("wprep1", i)) * 0.1
        W.view(-1)[::5] = dc.bf16_ties(W.view(-1)[::5].numel(), gen("ties1", i))
        n = taps * ci * co
        wf = torch.full((n + 64,), 7.0, dtype=BF, device=dev)
        wd = torch.full((n + 64,), 7.0, dtype=BF, device=dev)
        Wd = W.to(dev)
        _ffi.check(lib.rpc_dense_wprep(_ffi.ptr(Wd), kind, ci, co, taps, flip, _ffi.ptr(wf), _ffi.ptr(wd),
                                       _ffi.stream_of(wf)), "rpc_dense_wprep")
        torch.cuda.synchronize()
        rf, rd = dc.wprep_ref(W, kind, co, flip)
        assert torch.equal(raw(wf[:n]), raw(rf.to(BF).flatten())), i
        assert torch.equal(raw(wd[:n]), raw(rd.to(BF).flatten())), i
        assert (wf[n:] == 7.0).all() and (wd[n:] == 7.0).all(), i
