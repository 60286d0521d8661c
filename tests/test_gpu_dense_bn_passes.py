"""The dense engine's elementwise BatchNorm passes alone through the C ABI, bf16 images (perf mode):
rpc_dense_bn_apply, rpc_dense_bnbwd_stats and rpc_dense_bnbwd_apply, element by element against the float64
references of tests/_dense_cases.py. The check_* helpers take the engine, so test_gpu_dense_f32_kernels.py runs the
same checks on the fp32 entries.

Shapes. C in {8, 64, 128, 256, 384, 2048} (at 384, C / 8 = 48 channel groups leave 16 threads of a block without a
row lane; at 2048 a block is one row lane), M in {0, 1, 7, 255, 257, 4099} (the largest M not at C = 2048), both row
mappings of knob 9, which must give the same bits. Outputs go into [M][2C + 8] at channel offset C + 8 and dh is read
from such a slice (the FPN concat), inside a sentinel fill that must survive; z holds bf16 values whose
pre-activation is at least 1e-3 from zero, so the kernels' ReLU decisions are float64's and no entry is excused.

Bounds, u = 2^-24, derived from the kernels' arithmetic and not from what they give:
    bn_apply      |got - ref| <= 2^-8 |ref| + 4 u (|z - mean| |scale| + |beta|): the subtraction and the fused
                  multiply-add round once each, then one rounding to bf16 (fp32 images: the second term alone)
    bnbwd_stats   the float64 sum of the partial rows within (M + 16) u sum |term| of the float64 sums of
                  dm = dh [pre > 0] and dm xhat: xhat's two roundings, the product's, and M additions
                  (fp32 images, double rows: each row within (M + 8) 2^-53 of its own terms' magnitudes)
    bnbwd_apply   |got - ref| <= 2^-8 |ref| + 8 u |gi| (|dm| + |m1| + |xhat m2|): six fp32 roundings, one to bf16

Measured on the MI355X (the module prints them when it ends; 106 tests in 3 s): worst err / tol per entry
    rpc_dense_bn_apply              0.996   (fp32 images, second term alone: 0.48)
    rpc_dense_bnbwd_stats totals    0.13    (fp32 images, double rows: 0.17 of the 2^-53 bound per row)
    rpc_dense_bnbwd_apply           0.996   (fp32 images: 0.39)
The 0.996 is the rounding to bf16 itself and no missed term: half an ulp is 2^-8 of the lower end of a binade, so a
near-tie just above a power of two uses all of the first term, and among some 10^7 stored elements there are such.
The fp32 term stays below half of its bound, as the fp32 images show. No case misses its bound.
Mutants that stay in bounds, one build and one run of this module each: k_bn_apply reading bn[3C + c] in place of
bn[c] fails test_bn_apply_bf16 at every M > 0 (29 of 35); k_bnbwd_apply without its m2 term fails
test_bnbwd_apply_bf16 at every M > 0 (29 of 35).
"""
import collections
import zlib

import pytest
import torch

from robustpointclouds_amd import _ffi
from tests import _dense_cases as dc

pytestmark = pytest.mark.gpu

U = dc.U
SPARE = 3                                  # sentinel rows after every output image
WORST = {}
Eng = collections.namedtuple("Eng", "name dt apply stats bapply part_dt rnd")
BF16 = Eng("bf16", torch.bfloat16, "rpc_dense_bn_apply", "rpc_dense_bnbwd_stats", "rpc_dense_bnbwd_apply",
           torch.float32, 2.0 ** -8)
F32 = Eng("f32", torch.float32, "rpc_dense_bn_apply_f32", "rpc_dense_bnbwd_stats_f32", "rpc_dense_bnbwd_apply_f32",
          torch.float64, 0.0)


def report(worst):
    for k in sorted(worst):
        print(f"\nworst err/tol  {k:44s} {worst[k]:.4f}", end="")
    print()


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    report(WORST)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def within(got, ref, tol, what, entry, worst):
    err = (got - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    fin = ratio[torch.isfinite(ratio) & (tol > 0)]
    if fin.numel():
        worst[entry] = max(worst.get(entry, 0.0), float(fin.max()))
    bad = ~(err <= tol)                    # a NaN counts as bad
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), float(ratio[bad].max()))


def raw(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def draw(eng, shape, g, scale=1.0):
    """values of the engine's image type: the bf16 grid, or all 24 bits of fp32"""
    return (torch.randn(shape, generator=g) * scale).to(eng.dt)


class knob:
    """rpc_dense_tune(k, v), restored on exit"""

    def __init__(self, lib, k, v):
        self.lib, self.k, self.v = lib, k, v

    def __enter__(self):
        self.old = self.lib.rpc_dense_tune(self.k, self.v)
        assert self.lib.rpc_dense_tune(self.k, -1) == self.v

    def __exit__(self, *a):
        self.lib.rpc_dense_tune(self.k, self.old)


def check_bn_apply(lib, eng, C, M, worst):
    dev = torch.device("cuda")
    g = gen("apply", eng.name, C, M)
    bn = dc.bn_vec(C, g)
    z = dc.decisive_z(M, bn, g, eng.dt)
    ref, mag = dc.bn_apply_ref(z, bn)
    zd, bd = z.to(dev), bn.to(dev)
    pitch, off = 2 * C + 8, C + 8
    outs = []
    for v in (0, 1):
        what = f"{eng.apply} C {C} M {M} knob9 {v}"
        out = dc.sentinel_buffer(M + SPARE, pitch, eng.dt).to(dev)
        with knob(lib, 9, v):
            _ffi.check(getattr(lib, eng.apply)(_ffi.ptr(zd), M, C, _ffi.ptr(bd), _ffi.ptr(out), pitch, off,
                                               _ffi.stream_of(out)), what)
            torch.cuda.synchronize()
        assert dc.outside_unchanged(out, M, C, off), what
        got = dc.unpack(out, M, C, off).cpu()
        within(got.double(), ref, eng.rnd * ref.abs() + 4 * U * mag, what, eng.apply, worst)
        assert ((got == 0) == (ref == 0)).all(), what           # the ReLU clips exactly where float64's does
        outs.append(raw(got))
    assert torch.equal(outs[0], outs[1]), (eng.apply, C, M)
    if M >= 255:
        assert (ref == 0).any() and (ref > 0).any()


def run_stats(lib, eng, dhd, pitch, off, zd, M, C, bd):
    nb = lib.rpc_dense_bnbwd_blocks(M)
    assert nb == max((M + 255) // 256, 1)
    part = torch.full((nb + 1, 2 * C), float("nan"), dtype=eng.part_dt, device=zd.device)
    _ffi.check(getattr(lib, eng.stats)(_ffi.ptr(dhd), pitch, off, _ffi.ptr(zd), M, C, _ffi.ptr(bd), _ffi.ptr(part),
                                       _ffi.stream_of(part)), eng.stats)
    torch.cuda.synchronize()
    assert torch.isnan(part[nb]).all() and torch.isfinite(part[:nb]).all(), (eng.stats, C, M)
    return part[:nb].cpu().double()


def stats_case(eng, C, M, tag):
    g = gen(tag, eng.name, C, M)
    bn = dc.bn_vec(C, g)
    z = dc.decisive_z(M, bn, g, eng.dt)
    dh = draw(eng, (M, C), g)
    return g, bn, z, dh


def check_bnbwd_stats(lib, eng, C, M, worst):
    dev = torch.device("cuda")
    g, bn, z, dh = stats_case(eng, C, M, "stats")
    pitch, off = 2 * C + 8, C + 8
    dm, dmx = dc.bnbwd_terms(dh, z, bn)
    what = f"{eng.stats} C {C} M {M}"
    rows = run_stats(lib, eng, dc.pack(dh, pitch, off, SPARE).to(dev), pitch, off, z.to(dev), M, C, bn.to(dev))
    if M == 0:
        assert rows.shape[0] == 1 and (rows == 0).all(), what
        return
    tot = rows.sum(0)
    within(tot[:C], dm.sum(0), (M + 16) * U * dm.abs().sum(0), what + " sum dm", eng.stats + " totals", worst)
    within(tot[C:], dmx.sum(0), (M + 16) * U * dmx.abs().sum(0), what + " sum dm xhat", eng.stats + " totals", worst)
    if M >= 255:
        assert (dm == 0).any() and (dm != 0).any()
    return rows, dm, dmx


def check_bnbwd_apply(lib, eng, C, M, worst):
    dev = torch.device("cuda")
    g, bn, z, dh = stats_case(eng, C, M, "bapply")
    bnb = dc.bnb_vec(C, bn, g)
    bnb[3 * C:4 * C] += 0.01                                    # bnb's own mean: not the forward vector's
    ref, mag = dc.bnbwd_apply_ref(dh, z, bn, bnb)
    pitch, off = 2 * C + 8, C + 8
    dhd, zd, bd, bbd = dc.pack(dh, pitch, off, SPARE).to(dev), z.to(dev), bn.to(dev), bnb.to(dev)
    outs = []
    for v in (0, 1):
        what = f"{eng.bapply} C {C} M {M} knob9 {v}"
        dz = dc.sentinel_buffer(M + SPARE, C, eng.dt).to(dev)
        with knob(lib, 9, v):
            _ffi.check(getattr(lib, eng.bapply)(_ffi.ptr(dhd), pitch, off, _ffi.ptr(zd), M, C, _ffi.ptr(bd),
                                                _ffi.ptr(bbd), _ffi.ptr(dz), _ffi.stream_of(dz)), what)
            torch.cuda.synchronize()
        assert dc.outside_unchanged(dz, M, C, 0), what
        got = dz[:M].cpu()
        within(got.double(), ref, eng.rnd * ref.abs() + 8 * U * mag, what, eng.bapply, worst)
        outs.append(raw(got))
    assert torch.equal(outs[0], outs[1]), (eng.bapply, C, M)


def check_bn_guards(lib, eng):
    """declined before any launch, with valid pointers; nothing is written"""
    dev = torch.device("cuda")
    C, M = 16, 5
    z = torch.zeros((M, 64), dtype=eng.dt, device=dev)
    bn = torch.ones(4 * 2064, device=dev)
    bnb = torch.ones(5 * 2064, device=dev)
    out = dc.sentinel_buffer(M, 4200, eng.dt).to(dev)
    part = torch.full((2, 2 * 2064), float("nan"), dtype=eng.part_dt, device=dev)
    P, st = _ffi.ptr, _ffi.stream_of(z)
    apply_, stats, bapply = getattr(lib, eng.apply), getattr(lib, eng.stats), getattr(lib, eng.bapply)
    bad_c = [0, 4, 12, 2056]                                    # c < 8, c % 8, c > 2048
    for c in bad_c:
        assert apply_(P(z), M, c, P(bn), P(out), 4200, 0, st) == dc.RPC_ERR_ARG, c
        assert stats(P(z), 64, 0, P(z), M, c, P(bn), P(part), st) == dc.RPC_ERR_ARG, c
        assert bapply(P(z), 64, 0, P(z), M, c, P(bn), P(bnb), P(out), st) == dc.RPC_ERR_ARG, c
    for pitch, off in ((36, 0), (40, 4), (44, 12)):             # pitch or offset not a multiple of 8
        assert apply_(P(z), M, C, P(bn), P(out), pitch, off, st) == dc.RPC_ERR_ARG, (pitch, off)
        assert stats(P(z), pitch, off, P(z), M, C, P(bn), P(part), st) == dc.RPC_ERR_ARG, (pitch, off)
        assert bapply(P(z), pitch, off, P(z), M, C, P(bn), P(bnb), P(out), st) == dc.RPC_ERR_ARG, (pitch, off)
    for pitch, off in ((8, 0), (16, 8), (24, 16)):              # out_pitch < out_offset + c
        assert apply_(P(z), M, C, P(bn), P(out), pitch, off, st) == dc.RPC_ERR_ARG, (pitch, off)
    assert apply_(P(z), -1, C, P(bn), P(out), 16, 0, st) == dc.RPC_ERR_ARG
    torch.cuda.synchronize()
    assert dc.is_sentinel(out).all() and torch.isnan(part).all()


# ------------------------------------------------------------------ the bf16 engine
@pytest.mark.parametrize("C,M", dc.bn_shapes())
def test_bn_apply_bf16(C, M):
    check_bn_apply(_ffi.load(), BF16, C, M, WORST)


@pytest.mark.parametrize("C,M", dc.bn_shapes())
def test_bnbwd_stats_bf16(C, M):
    check_bnbwd_stats(_ffi.load(), BF16, C, M, WORST)


@pytest.mark.parametrize("C,M", dc.bn_shapes())
def test_bnbwd_apply_bf16(C, M):
    check_bnbwd_apply(_ffi.load(), BF16, C, M, WORST)


def test_bn_pass_argument_guards_bf16():
    check_bn_guards(_ffi.load(), BF16)
