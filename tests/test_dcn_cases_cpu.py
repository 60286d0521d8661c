"""Pins tests/_dcn_cases.py on the CPU: the explicit restatement of the deformable convolution and of mmcv
get_coordinate_weight against oracle/dcn.py and torch autograd on every case of the lists (integer positions and every
probe included), the magnitudes, the representability the dyadic families rely on (asserted inside reference() by
round trips), the sample-class floors and the bf16 interval criterion."""
import pytest
import torch
import torch.nn.functional as F

from tests import _dcn_cases as dn

GROUPS = sorted({(f, s) for f, s, _ in dn.dyadic_cases()})
NAMES = ("out", "dx", "doff", "dob", "dW")


def _patterns(family, shape):
    return [p for f, s, p in dn.dyadic_cases() if (f, s) == (family, shape)]


@pytest.mark.parametrize("family,shape", GROUPS)
def test_reference_of_every_dyadic_case(family, shape):
    """reference() itself asserts: inputs on the grid, col / dcol / bilinear weights bf16 numbers, outputs fp32
    numbers, explicit == autograd exactly, every magnitude below 2^24 grid units. Here: the magnitudes dominate, the
    padded probes' properties."""
    B, H, W = shape
    for p in _patterns(family, shape):
        r = dn.reference(family, shape, p)
        for n in NAMES:
            assert bool((getattr(r, "m_" + n) >= getattr(r, n).abs()).all()), (p, n)
        c = dn.make_case(family, shape, p)
        if p[0] == "zero":           # a plain grouped 3 x 3 convolution
            assert torch.equal(r.out, F.conv2d(c.x, c.W, padding=1, groups=4))
            assert float(r.doff.abs().max()) > 0       # one-sided coordinate weights on integer positions
        if p[0] == "far":            # everything invalid
            for n in NAMES:
                assert float(getattr(r, n).abs().max()) == 0.0 and float(getattr(r, "m_" + n).max()) == 0.0, (p, n)
            assert float(r.hits.max()) == 0.0
        if p[0] == "converge":
            cy, cx = dn.converge_pixel(p[1], shape)
            assert bool((r.hits[:, cy, cx] == KT_HITS(H, W)).all())
            g = c.gout.reshape(B, 4, 16, H * W).sum(3)                          # every tap reads x[:, :, cy, cx]
            want = torch.einsum("goci,bgo->bgc", c.W.reshape(4, 16, 16, 9), g).reshape(B, 64)
            assert torch.equal(r.dx[:, :, cy, cx], want)


def KT_HITS(H, W):
    return float(dn.KT * H * W)


@pytest.mark.parametrize("shape", dn.GENERIC_SHAPES)
def test_explicit_equals_autograd_generic(shape):
    c = dn.make_case("generic", shape, dn.RANDOM)
    a = dn.autograd_ref(c)
    e = dn.explicit(c.x, dn.total_offsets(c), c.W, c.gout)
    r = dn.reference("generic", shape, dn.RANDOM)
    for n in NAMES:
        assert float((a[n] - e[n]).abs().max()) <= 1e-12 * float(a[n].abs().max()), n
        assert bool((getattr(r, "m_" + n) >= a[n].abs() * (1 - 1e-12)).all()), n
    cls = dn.classify(dn.total_offsets(c), shape)
    assert cls["invalid"] > 0 and cls["valid_partial"] > 0


def test_class_floors():
    """the random draw at (2, 16, 24) holds at least CLASS_FLOOR samples of every class, on both families"""
    for f in dn.DYADIC:
        c = dn.make_case(f, (2, 16, 24), dn.RANDOM)
        n = dn.classify(dn.total_offsets(c), c.shape)
        print(f, n)
        assert set(n) == set(dn.CLASSES)
        for k, v in n.items():
            assert v >= dn.CLASS_FLOOR, (f, k, v)
        assert n["window_in"] + n["window_out"] + n["window_mixed"] == 2 * 16 * 24 * 9 - n["invalid"]


def test_probe_coverage():
    """what each probe is for, counted: the edge probes put whole tap rows exactly on an edge, the half-integer edge
    probes give valid samples with corners outside, shifts beyond the window's design limit split (3/2, 2) or lose
    (3) the window; at one tile the window holds the whole image"""
    def cls(shape, p, f="halves"):
        return dn.classify(dn.total_offsets(dn.make_case(f, shape, p)), shape)

    for shape in dn.PROBE_SHAPES:
        B, H, W = shape
        n = cls(shape, ("row", "-1"))
        assert n["on_edge"] >= 3 * B * H * W and n["invalid"] >= 3 * B * H * W     # tap row 0 on -1
        assert cls(shape, ("row", "n"))["invalid"] == 9 * B * H * W
        assert cls(shape, ("col", "n"))["on_edge"] >= 3 * B * H * W
        for e in ("-1/2", "n-1/2"):
            assert cls(shape, ("row", e))["valid_partial"] >= 3 * B * H * (W - 2)
            assert cls(shape, ("col", e))["valid_partial"] >= 3 * B * (H - 2) * W
        assert cls(shape, ("row", "n-1"))["valid_integer"] >= 3 * B * H * (W - 2)
        assert cls(shape, ("zero",))["valid_integer"] == 9 * B * H * W - cls(shape, ("zero",))["invalid"]
    one = (1, 8, 8)
    for p in dn.probes("eighths"):
        n = cls(one, p, "eighths")
        assert n["window_out"] == 0 and n["window_mixed"] == 0, p
    big = (2, 16, 24)
    for a in (1.5, 2.0):
        for p in (("shift", a, 0.0), ("shift", 0.0, -a), ("shift", -a, -a)):
            assert cls(big, p)["window_mixed"] >= dn.CLASS_FLOOR, p
    for p in (("shift", 0.5, 0.0), ("shift", -1.0, -1.0), ("zero",)):
        n = cls(big, p)
        assert n["window_out"] == 0 and n["window_mixed"] == 0, p
    # exactly + 1 is past the design limit: the lower / right corners (weight 0) of the tile's last row / column
    # lie one past the window and go through the global path
    assert cls(big, ("shift", 1.0, 0.0))["window_mixed"] >= dn.CLASS_FLOOR
    for p in (("shift", 3.0, 0.0), ("shift", -3.0, 3.0)):
        assert cls(big, p)["window_out"] >= dn.CLASS_FLOOR, p
    assert cls(big, ("converge", "interior"))["window_out"] >= dn.CLASS_FLOOR


def test_case_lists():
    cases = dn.dyadic_cases()
    assert len(set(cases)) == len(cases)
    for f in dn.DYADIC:
        assert {s for ff, s, p in cases if ff == f and p == dn.RANDOM} == set(dn.SHAPES)
        for s in dn.PROBE_SHAPES:
            ps = [p for ff, ss, p in cases if (ff, ss) == (f, s) and p != dn.RANDOM]
            assert ps == dn.probes(f)
            shifts = {(p[1], p[2]) for p in ps if p[0] == "shift"}
            for a in (0.5, 1.0, 1.5, 2.0, 2.5, 3.0):
                for s_ in (a, -a):
                    assert {(s_, 0.0), (0.0, s_), (s_, s_)} <= shifts
    assert len({dn.case_id(c) for c in cases}) == len(cases)


def test_bf16_interval():
    g = dn.gen("interval")
    ref = torch.randn(4096, generator=g, dtype=torch.float64) * 40
    b = torch.rand(4096, generator=g, dtype=torch.float64) * 1e-3
    lo, hi = dn.bf16_interval(ref, b)
    assert bool((lo <= hi).all()) and dn.is_bf16(lo) and dn.is_bf16(hi)
    r = dn.bf16_round(ref)
    assert bool((lo <= r).all() and (r <= hi).all())                       # accepts bf16(ref)
    assert not dn.bad_entries(r, ref, b, True).any()
    lo2, hi2 = dn.bf16_interval(ref, 2 * b)                                # monotone in b
    assert bool((lo2 <= lo).all() and (hi2 >= hi).all())
    s = torch.sort(ref).values                                            # and in ref
    assert bool((dn.bf16_round(s)[1:] >= dn.bf16_round(s)[:-1]).all())
    # a one-unit error at |out| = 37 (bf16 spacing 1/4, bound far below it) is outside; so is a NaN
    ref37 = torch.tensor([37.0, -37.25, 36.75], dtype=torch.float64)
    b37 = torch.full((3,), 1e-3, dtype=torch.float64)
    assert not dn.bad_entries(ref37, ref37, b37, True).any()
    for d in (0.25, -0.25):
        assert dn.bad_entries(ref37 + d, ref37, b37, True).all()
    assert dn.bad_entries(torch.full((3,), float("nan"), dtype=torch.float64), ref37, b37, True).all()
    assert dn.bad_entries(ref37 + 2e-3, ref37, b37, False).all() and not dn.bad_entries(ref37 + 5e-4, ref37, b37,
                                                                                         False).any()


def test_bound_shapes_and_terms():
    shape = (1, 8, 8)
    r = dn.reference("halves", shape, dn.RANDOM)
    for n in NAMES:
        b = dn.bound(n, r, shape)
        assert b.shape == getattr(r, n).shape and bool((b >= 0).all())
    assert dn.terms("out", shape) == 148 and dn.terms("doff", shape) == 38
    assert dn.terms("dW", shape) == 68 and dn.terms("dob", shape) == 102
    assert float(r.hits.sum()) > 0 and float(dn.terms("dx", shape, r.hits).min()) >= 22
    # on the dyadic families the bound of out, dx and doff is below one grid unit, so the criterion alone is
    # exactness; the long sums (dW, dob, dx of the convergence probes) have bounds of several units, which is why the
    # GPU tests also demand equality there (reference() asserts the 2^24 condition that makes every sum exact)
    for f in dn.DYADIC:
        rr = dn.reference(f, (2, 16, 24), dn.RANDOM)
        units = dn._units(f)
        for n in ("out", "dx", "doff"):
            assert float(dn.bound(n, rr, (2, 16, 24)).max()) < units[n], (f, n)
        assert float(dn.bound("dob", rr, (2, 16, 24)).max()) > units["dob"]
