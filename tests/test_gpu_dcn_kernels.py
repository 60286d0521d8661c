"""The deformable-convolution kernels of csrc/dcn.hip alone through the C ABI, entry by entry against the float64
references of tests/_dcn_cases.py: rpc_dcn_prep_weight, rpc_dcn_forward + rpc_dcn_backward(_ex) (bf16 images, MFMA) and
rpc_dcn_forward_f32 + rpc_dcn_backward_f32(_ex) (fp32 parity mode).

Criterion, with u = 2^-24 and b = (terms + 8) u sum |a| |w| (terms derived in _dcn_cases.py):
    fp32 outputs   |got - ref| <= b
    bf16 outputs   bf16(ref - b) <= got <= bf16(ref + b)   (out and doff of the bf16 kernels)
On the two dyadic families every rounding inside the kernels is exact (asserted by round trips when the reference is
built) and every sum stays below 2^24 grid units, so fp32 accumulation is exact in any order: b is below one grid unit
for out, dx and doff, and the tests demand equality with float64 (after the one bf16 store rounding) on all six outputs.
A disagreement there is an indexing or semantics bug, never noise. The generic family (randn values, offsets on a
2^-10 grid so that every floor and validity decision agrees) holds the fp32 kernels to b with full 24-bit operands.

What the cases reach that a norm over the tensor cannot see: corners split between the 12 x 12 LDS window and global
memory (shifts of 3/2 and 2, the weight-0 corner of a shift of exactly 1), positions exactly on -1 / H / W (invalid)
and on -1/2 / H - 1/2 (valid, two corners outside), integer positions (weights 1, 0, 0, 0 with one-sided coordinate
weights), k_gather_dx with TY = 1 or TX = 1, samples below the last row of a frame, 9 H W contributions onto one input
pixel through the atomic path, dx accumulation over calls, pitched images between sentinels, a NaN-filled workspace.
No non-finite or astronomically large offsets: a test whose failure mode is a wild address does not belong here.

Measured on the MI355X (377 tests in 18 s, most of it the CPU references): every dyadic case equal to float64 on all
six outputs in both precisions; generic family worst err / tol out 0.019, dx 0.035, doff 0.009, dW 0.032, dob 0.0003.
No case misses its bound and no kernel bug was found. Value-only mutants of dcn.hip, one build and one run of this
module each (tests failing of 377): samp's lower corners tested with < for <= 285; k_bwd without the out-of-window
atomics 118 (shifts beyond 1, the random draws, the convergence probes; bf16 only); k_gather_dx with (y + 1) / TE 65;
dx[e] = s 126 (every case with out-of-window corners, whose atomics land before the gather, and test_dx_accumulates);
the out-of-window corner 4 given corner 3's weight 32; ph >= -1 226 (every case with a sample exactly on -1).
ph <= H was compiled and not run (it reads a row past the last frame): the row / col probes on n and the on-edge
samples of the random draws have frame 0 read frame 1's first row in the fp32 kernels, which changes out.
"""
import itertools

import pytest
import torch

from robustpointclouds_amd import _ffi
from tests import _dcn_cases as dn
from tests import _dense_cases as dc

pytestmark = pytest.mark.gpu

SPARE = 3                                   # sentinel rows after every output image
GUARD = 256                                 # bytes after the workspace that must stay untouched
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
PRECS = ("bf16", "f32")
NAMES = ("out", "dx", "doff", "dob", "dW")
WORST = {}
BIG, ONE = (2, 16, 24), (1, 8, 8)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for k in sorted(WORST):
        print(f"\nworst err/tol  {k:44s} {WORST[k]:.4f}", end="")
    print()


def _dev():
    return torch.device("cuda")


def raw(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def prep_weights(lib, W32):
    wf = torch.empty((9, 64, 64), dtype=torch.bfloat16, device=W32.device)
    wd = torch.empty((9, 64, 64), dtype=torch.bfloat16, device=W32.device)
    _ffi.check(lib.rpc_dcn_prep_weight(_ffi.ptr(W32), _ffi.ptr(wf), _ffi.ptr(wd), _ffi.stream_of(W32)), "prep")
    return wf, wd


def run(prec, case, xp=64, offp=64, offc=0, wide=None, op=64, dop=64, dx_buf=None, ws_fill=0, W=None, slice_j=None):
    """forward and backward of one case through the ABI. Every image lies in a sentinel fill (inputs too: a kernel
    that read a neighbouring column would return NaN); wide: a [pixels][offp] image that already holds the case's
    offsets at channel offc between other values; dx_buf: accumulate into this device buffer; slice_j: the offset
    gradient as 18 channels at channel 18 j of a 256-wide sentinel image (rpc_dcn_backward(_f32)_ex).
    -> ({name: CPU tensor}, the device buffers)"""
    lib, dev, dt = _ffi.load(), _dev(), DT[prec]
    B, H, Wd = case.shape
    M = B * H * Wd
    f32 = prec == "f32"
    xd = dc.pack(dn.to_rows(case.x).to(dt), xp, 0).to(dev)
    od = (dc.pack(dn.to_rows(case.off).to(dt), offp, offc) if wide is None else wide.to(dt)).to(dev)
    gd = dc.pack(dn.to_rows(case.gout).to(dt), dop, 0).to(dev)
    ob = case.ob.float().to(dev)
    W32 = (case.W if W is None else W).float().to(dev).contiguous()
    st = _ffi.stream_of(xd)
    wf, wb = (W32, W32) if f32 else prep_weights(lib, W32)
    out = dc.sentinel_buffer(M + SPARE, op, dt).to(dev)
    fwd = lib.rpc_dcn_forward_f32 if f32 else lib.rpc_dcn_forward
    _ffi.check(fwd(_ffi.ptr(xd), xp, _ffi.ptr(od[:, offc:]), offp, _ffi.ptr(ob), _ffi.ptr(wf), _ffi.ptr(out), op, B, H,
                   Wd, st), "forward " + prec)
    if dx_buf is None:
        dx_buf = torch.zeros((M + SPARE, 64), device=dev)
        dx_buf[M:] = float("nan")
    dfp, dfc, dch = (64, 0, 64) if slice_j is None else (256, 18 * slice_j, 18)
    doff = dc.sentinel_buffer(M + SPARE, dfp, dt).to(dev)
    dob = torch.full((18 + SPARE,), float("nan"), device=dev)
    dW = torch.full((64 * 16 * 9 + SPARE,), float("nan"), device=dev)
    wsz = lib.rpc_dcn_backward_workspace_size(B, H, Wd)
    tiles = M // 64
    assert wsz == 4 * (tiles * (9 * 1024 + 32) + 9 * 1024 + 32 + tiles * 144 * 64)
    ws = torch.full((wsz + GUARD,), ws_fill, dtype=torch.uint8, device=dev)
    head = (_ffi.ptr(xd), xp, _ffi.ptr(od[:, offc:]), offp, _ffi.ptr(ob), _ffi.ptr(wb), _ffi.ptr(gd), dop,
            _ffi.ptr(dx_buf), _ffi.ptr(doff[:, dfc:]), dfp)
    tail = (_ffi.ptr(dob), _ffi.ptr(dW), B, H, Wd, _ffi.ptr(ws), wsz, st)
    if slice_j is None:
        bwd = lib.rpc_dcn_backward_f32 if f32 else lib.rpc_dcn_backward
        _ffi.check(bwd(*head, *tail), "backward " + prec)
    else:
        bwd = lib.rpc_dcn_backward_f32_ex if f32 else lib.rpc_dcn_backward_ex
        _ffi.check(bwd(*head, dch, *tail), "backward_ex " + prec)
    torch.cuda.synchronize()
    what = (prec, dn.case_id(case[:3]), xp, offp, offc, op, dop, slice_j)
    assert dc.outside_unchanged(out, M, 64, 0), what              # columns past 64 and the spare rows
    assert not dc.is_sentinel(out[:M, :64]).any(), what
    assert dc.outside_unchanged(doff, M, dch, dfc), what
    assert not dc.is_sentinel(doff[:M, dfc:dfc + dch]).any(), what
    assert torch.isnan(dx_buf[M:]).all() and torch.isfinite(dx_buf[:M]).all(), what
    assert torch.isnan(dob[18:]).all() and torch.isnan(dW[64 * 16 * 9:]).all(), what
    assert (ws[wsz:] == ws_fill).all(), what                      # the stated workspace size is honoured
    res = {"out": out[:M, :64].cpu(), "dx": dx_buf[:M].cpu(), "doff": doff[:M, dfc:dfc + dch].cpu(),
           "dob": dob[:18].cpu(), "dW": dW[:64 * 16 * 9].view(64, 16, 3, 3).cpu()}
    return res, {"out": out, "dx": dx_buf, "doff": doff, "dob": dob, "dW": dW, "ws": ws}


def as_ref_layout(name, t, shape):
    t = t.double()
    return dn.to_nchw(t, shape) if name in ("out", "dx", "doff") else t


def hold(prec, got, ref, shape, what, exact, dx_base=None):
    """all six outputs against the criterion; exact (dyadic families): also equal to float64, bf16 outputs after the
    one store rounding. dx_base: what dx held before the call(s) (one more term, its magnitude added)."""
    for name in NAMES:
        g = as_ref_layout(name, got[name], shape)
        r, b = getattr(ref, name), dn.bound(name, ref, shape)
        if name == "doff" and g.shape[1] > 18:
            assert float(g[:, 18:].abs().max()) == 0.0, (what, prec, "doff channels 18..63")
            g = g[:, :18]
        if name == "dx" and dx_base is not None:
            r = r + dx_base
            b = (dn.terms("dx", shape, ref.hits) + 1 + 8) * dn.U * (ref.m_dx + dx_base.abs())
        is_bf16 = prec == "bf16" and name in ("out", "doff")
        bad =dn.bad_entries(g, r, b, is_bf16)
        if bad.any():
            idx = bad.nonzero()[0].tolist()
            raise AssertionError((what, prec, name, int(bad.sum()), "first", idx, float(g[tuple(idx)]),
                                  float(r[tuple(idx)]), "worst", float((g - r).abs()[bad].max())))
        if not is_bf16:
            ratio = ((g - r).abs() / b.clamp_min(1e-300))[b > 0]
            if ratio.numel():
                key = f"{prec} {name} ({'dyadic' if exact else 'generic'})"
                WORST[key] = max(WORST.get(key, 0.0), float(ratio.max()))
        if exact:
            want = dn.bf16_round(r) if is_bf16 else r
            ne = g != want
            if ne.any():
                idx = ne.nonzero()[0].tolist()
                raise AssertionError((what, prec, name, "not exact", int(ne.sum()), "first", idx, float(g[tuple(idx)]),
                                      float(want[tuple(idx)])))


# ------------------------------------------------------------------ 1. forward and backward, dyadic families
@pytest.mark.parametrize("case", dn.dyadic_cases(), ids=dn.case_id)
def test_dyadic_matches_fp64(case):
    family, shape, pattern = case
    c = dn.make_case(*case)
    ref = dn.reference(*case)
    for prec in PRECS:
        got, _ = run(prec, c)
        hold(prec, got, ref, shape, dn.case_id(case), exact=True)
        if pattern[0] == "far":                                    # everything invalid: exactly zero
            for n in NAMES:
                assert float(got[n].float().abs().max()) == 0.0, (prec, n)


# ------------------------------------------------------------------ 2. generic family, fp32 kernels
@pytest.mark.parametrize("shape", dn.GENERIC_SHAPES)
def test_generic_f32_matches_fp64(shape):
    c = dn.make_case("generic", shape, dn.RANDOM)
    got, _ = run("f32", c)
    hold("f32", got, dn.reference("generic", shape, dn.RANDOM), shape, f"generic {shape}", exact=False)


# ------------------------------------------------------------------ 3. weight prep, bit for bit
@pytest.mark.parametrize("values", ["randn", "ties"])
def test_prep_weight_bit_exact(values):
    """wf [9][co][ci] and wd [9][ci][co]: W.to(bfloat16) (round to nearest even) placed by index inside the four
    diagonal 16 x 16 group blocks, + 0 elsewhere"""
    lib, dev = _ffi.load(), _dev()
    g = dn.gen("prep", values)
    W = torch.randn((64, 16, 3, 3), generator=g) * 0.1
    if values == "ties":
        W.view(-1)[::3] = dc.bf16_ties(W.view(-1)[::3].numel(), g)
    Wb = W.to(torch.bfloat16).reshape(64, 16, 9)
    want_f = torch.zeros((9, 64, 64), dtype=torch.bfloat16)
    for q in range(4):
        want_f[:, 16 * q:16 * q + 16, 16 * q:16 * q + 16] = Wb[16 * q:16 * q + 16].permute(2, 0, 1)
    want_d = want_f.transpose(1, 2).contiguous()
    n = 9 * 64 * 64
    wf = dc.sentinel_buffer(1, n + 64, torch.bfloat16).to(dev)
    wd = dc.sentinel_buffer(1, n + 64, torch.bfloat16).to(dev)
    Wd = W.to(dev)
    _ffi.check(lib.rpc_dcn_prep_weight(_ffi.ptr(Wd), _ffi.ptr(wf), _ffi.ptr(wd), _ffi.stream_of(Wd)), "prep")
    torch.cuda.synchronize()
    assert torch.equal(raw(wf[0, :n]), raw(want_f.flatten()))
    assert torch.equal(raw(wd[0, :n]), raw(want_d.flatten()))
    assert dc.is_sentinel(wf[0, n:]).all() and dc.is_sentinel(wd[0, n:]).all()
    assert int((raw(want_f) == 0).sum()) >= n * 3 // 4            # the off-diagonal blocks: + 0 bit patterns
    for args in ((None, wf, wd), (Wd, None, wd), (Wd, wf, None)):  # refused: a null pointer
        before = raw(wf).clone(), raw(wd).clone()
        assert lib.rpc_dcn_prep_weight(*[_ffi.ptr(a) for a in args], _ffi.stream_of(Wd)) == dn.RPC_ERR_ARG
        torch.cuda.synchronize()
        assert torch.equal(raw(wf), before[0]) and torch.equal(raw(wd), before[1])


# ------------------------------------------------------------------ 4. dx accumulates
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", [("halves", BIG, dn.RANDOM), ("eighths", ONE, ("converge", "corner"))], ids=dn.case_id)
def test_dx_accumulates(prec, key):
    """CenterHeadFn.backward runs 12 DCN backwards into one buffer: a call adds to what dx holds. Prefill with a
    dyadic pattern -> prefill + grad exactly; a second call with other weights into the same buffer -> the sum."""
    c, ref = dn.make_case(*key), dn.reference(*key)
    B, H, W = c.shape
    M = B * H * W
    g = dn.gen("prefill", key)
    pre = torch.randint(-64, 65, (M, 64), generator=g).double() / 8
    buf = torch.full((M + SPARE, 64), float("nan"), device=_dev())
    buf[:M] = pre.float().to(_dev())
    got, _ = run(prec, c, dx_buf=buf)
    base = dn.to_nchw(pre, c.shape)
    hold(prec, got, ref, c.shape, "prefilled " + dn.case_id(key), exact=True, dx_base=base)
    W2 = c.W.flip(0).roll(1, 1).contiguous()
    assert not torch.equal(W2, c.W)
    e2 = dn.explicit(c.x, dn.total_offsets(c), W2, c.gout)
    got2, _ = run(prec, c, dx_buf=buf, W=W2)
    want = base + ref.dx + e2["dx"]
    assert dn.is_f32(want)
    assert torch.equal(as_ref_layout("dx", got2["dx"], c.shape), want)


# ------------------------------------------------------------------ 5. pitches and slices, sentinel neighbours
def _same_bits(a, b, what):
    for n in NAMES:
        assert torch.equal(raw(a[n]), raw(b[n])), (what, n)


@pytest.mark.parametrize("prec", PRECS)
def test_pitched_images_equal_packed(prec):
    """xp, op, dop in {64, 72, 128}: every output bit for bit that of the packed call; run() asserts that the columns
    past 64 of the pitched output and the rows after it keep their sentinel (the input images' spare columns hold NaN)"""
    c = dn.make_case("halves", BIG, dn.RANDOM)
    base, _ = run(prec, c)
    hold(prec, base, dn.reference("halves", BIG, dn.RANDOM), BIG, "packed", exact=True)
    for xp, op, dop in itertools.product((64, 72, 128), repeat=3):
        if (xp, op, dop) != (64, 64, 64):
            got, _ = run(prec, c, xp=xp, op=op, dop=dop)
            _same_bits(got, base, (xp, op, dop))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("j", [0, 5, 13])
def test_offset_slice_of_shared_image(prec, j):
    """the head's concatenated offset conv: forward and backward read their offsets at channel 18 j of a 256-wide
    image whose other channels hold other DCNs' offsets, and the 18 offset gradients go to channel 18 j of a 256-wide
    image; bit for bit the packed call, every other column unchanged"""
    key = ("eighths", BIG, dn.RANDOM)
    c = dn.make_case(*key)
    M = BIG[0] * BIG[1] * BIG[2]
    g = dn.gen("wide", j)
    wide = torch.randint(-24, 25, (M, 256), generator=g).double() / 8           # other offsets, within +-3
    wide[:, 18 * j:18 * j + 18] = dn.to_rows(c.off)
    assert dn.is_bf16(wide)
    base, _ = run(prec, c)
    got, _ = run(prec, c, offp=256, offc=18 * j, wide=wide)
    _same_bits(got, base, ("wide offsets", j))
    got, _ = run(prec, c, offp=256, offc=18 * j, wide=wide, slice_j=j)
    assert got["doff"].shape == (M, 18)
    assert torch.equal(raw(got["doff"]), raw(base["doff"][:, :18])), j
    for n in ("out", "dx", "dob", "dW"):
        assert torch.equal(raw(got[n]), raw(base[n])), (j, n)
    if j == 5:
        hold(prec, base, dn.reference(*key), BIG, "slice base", exact=True)


# ------------------------------------------------------------------ 6. workspace
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", [("halves", BIG, dn.RANDOM), ("halves", ONE, ("shift", 1.5, 1.5))], ids=dn.case_id)
def test_workspace_needs_no_initialisation(prec, key):
    """a workspace of exactly the stated size filled with 0xFF bytes (NaN) gives the bits of a zeroed one"""
    c = dn.make_case(*key)
    zero, _ = run(prec, c, ws_fill=0)
    nan, _ = run(prec, c, ws_fill=0xFF)
    _same_bits(nan, zero, key)
    hold(prec, nan, dn.reference(*key), c.shape, "NaN workspace", exact=True)


# ------------------------------------------------------------------ 7. argument checks
def _arg_sets(prec):
    """valid argument lists of the forward and the backward entry, and every refused variation with its code"""
    lib, dev, dt = _ffi.load(), _dev(), DT[prec]
    f32 = prec == "f32"
    B, H, W = 1, 8, 8
    M = B * H * W
    P = 136
    x = torch.zeros((M, P), dtype=dt, device=dev)
    ob = torch.zeros(18, device=dev)
    Wt = torch.zeros((64, 16, 3, 3), device=dev)
    w = Wt if f32 else torch.zeros((9, 64, 64), dtype=torch.bfloat16, device=dev)
    outs = {"out": dc.sentinel_buffer(M, P, dt).to(dev), "doff": dc.sentinel_buffer(M + 1, P, dt).to(dev),
            "dx": torch.full((M, 64), float("nan"), device=dev), "dob": torch.full((18,), float("nan"), device=dev),
            "dW": torch.full((64 * 16 * 9,), float("nan"), device=dev)}
    wsz = lib.rpc_dcn_backward_workspace_size(B, H, W)
    ws = torch.full((wsz,), 0xA5, dtype=torch.uint8, device=dev)
    st = _ffi.stream_of(x)
    p = _ffi.ptr
    fwd = dict(x=p(x), xp=64, off=p(x), offp=64, ob=p(ob), w=p(w), out=p(outs["out"]), op=P, B=B, H=H, W=W, st=st)
    bwd = dict(x=p(x), xp=64, off=p(x), offp=64, ob=p(ob), w=p(w), dout=p(x), dop=64, dx=p(outs["dx"]),
               doff=p(outs["doff"]), doffp=64, dob=p(outs["dob"]), dW=p(outs["dW"]), B=B, H=H, W=W, ws=p(ws), wsz=wsz,
               st=st)
    geo = [dict(H=12), dict(W=12), dict(H=4), dict(W=20), dict(B=0), dict(H=0), dict(B=-1)]
    A, S = dn.RPC_ERR_ARG, dn.RPC_ERR_UNSUPPORTED
    bad_f = [(g, S) for g in geo] + [({k: None}, A) for k in ("x", "off", "ob", "w", "out")]
    bad_b = [(g, S) for g in geo] + [({k: None}, A) for k in ("x", "off", "ob", "w", "dout", "dx", "doff", "dob", "dW",
                                                               "ws")]
    low, odd = (56, 68) if not f32 else (60, 66)                 # below 64; not a multiple of 8 (bf16) / 4 (fp32)
    bad_f += [(dict(xp=low), A), (dict(xp=odd), A), (dict(op=low), A), (dict(op=odd), A), (dict(offp=16), A)]
    bad_b += [(dict(xp=low), A), (dict(xp=odd), A), (dict(dop=low), A), (dict(dop=odd), A), (dict(offp=16), A)]
    if f32:
        bad_f += [(dict(offp=17), A)]
        bad_b += [(dict(offp=17), A), (dict(doffp=16), A), (dict(doffp=66), A)]
        mis = outs["doff"].view(-1)[1:]                          # 4 bytes off a 16-byte boundary
    else:
        bad_f += [(dict(offp=20), A)]
        bad_b += [(dict(offp=20), A), (dict(doffp=56), A), (dict(doffp=68), A)]
        mis = outs["doff"].view(-1)[4:]                          # 8 bytes off
    bad_b += [(dict(doff=p(mis)), A), (dict(wsz=wsz - 1), dn.RPC_ERR_WORKSPACE), (dict(wsz=0), dn.RPC_ERR_WORKSPACE)]
    return fwd, bad_f, bwd, bad_b, outs, ws


@pytest.mark.parametrize("prec", PRECS)
def test_argument_checks_leave_outputs_alone(prec):
    lib = _ffi.load()
    f32 = prec == "f32"
    fwd, bad_f, bwd, bad_b, outs, ws = _arg_sets(prec)
    f_fn = lib.rpc_dcn_forward_f32 if f32 else lib.rpc_dcn_forward
    b_fn = lib.rpc_dcn_backward_f32 if f32 else lib.rpc_dcn_backward
    for change, code in bad_f:
        assert f_fn(*{**fwd, **change}.values()) == code, ("forward", change)
    for change, code in bad_b:
        assert b_fn(*{**bwd, **change}.values()) == code, ("backward", change)
    for ch in (20, 64 + 8, 0):                                    # _ex: a channel count that is neither 18 nor 64
        a = dict(bwd)
        args = list(a.values())
        args.insert(11, ch)
        fn = lib.rpc_dcn_backward_f32_ex if f32 else lib.rpc_dcn_backward_ex
        assert fn(*args) == dn.RPC_ERR_ARG, ch
    assert lib.rpc_dcn_backward_workspace_size(1, 12, 8) == 0 and lib.rpc_dcn_backward_workspace_size(0, 8, 8) == 0
    torch.cuda.synchronize()
    for n, t in outs.items():
        assert dc.is_sentinel(t).all(), n
    assert (ws == 0xA5).all()
    # the unchanged lists are accepted
    _ffi.check(f_fn(*fwd.values()), "forward")
    _ffi.check(b_fn(*bwd.values()), "backward")
    torch.cuda.synchronize()
    assert not dc.is_sentinel(outs["out"][:, :64]).any() and dc.is_sentinel(outs["out"][:, 64:]).all()


# ------------------------------------------------------------------ 8. determinism
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("family", dn.DYADIC)
def test_two_runs_are_bit_identical(prec, family):
    for shape, pattern in ((BIG, dn.RANDOM), (BIG, ("shift", 2.0, 2.0)), ((1, 32, 8), dn.RANDOM)):
        c = dn.make_case(family, shape, pattern)
        a, _ = run(prec, c)
        b, _ = run(prec, c)
        _same_bits(a, b, (family, shape, pattern))


def test_two_runs_generic_f32():
    """everything but dx bit for bit; dx goes through float atomics there (summation order) and is held to the
    bound in both runs"""
    c = dn.make_case("generic", BIG, dn.RANDOM)
    ref = dn.reference("generic", BIG, dn.RANDOM)
    a, _ = run("f32", c)
    b, _ = run("f32", c)
    for n in ("out", "doff", "dob", "dW"):
        assert torch.equal(raw(a[n]), raw(b[n])), n
    hold("f32", a, ref, BIG, "generic run 1", exact=False)
    hold("f32", b, ref, BIG, "generic run 2", exact=False)
