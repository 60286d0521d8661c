"""Inputs, float64 references and bounds for the deformable-convolution kernel tests (csrc/dcn.hip):
test_dcn_cases_cpu.py pins them on the CPU, test_gpu_dcn_kernels.py holds the kernels to them. No GPU import:
tensors are NCHW float64 on the CPU; to_rows / to_nchw convert to the kernels' [pixel][channel] images.

Why the inputs are dyadic. The bf16 kernels round col, dcol and the bilinear weights of S_k to bf16; against random
data float64 can be met only to about 2^-8 sum |a| |w|, the size of one missing corner term, which is useless. On the
two families below nothing is lost at any of those points (reference() asserts it by round trips, it is not assumed):
every col and dcol value and every bilinear weight is a bf16 number, every output and every sum |a| |w| stays far
below 2^24 units of its grid, so fp32 accumulation is exact in any order (MFMA, shuffles, atomics, the slab reduce).
The only rounding left is the bf16 store of out and doff, and the bound (terms + 8) u sum |a| |w| is in effect
exactness: a disagreement is an indexing or semantics bug, never noise.

    family    offsets and offset bias    x                   W                       dOut
    halves    multiples of 1/2           integers in [-8, 8]  integers in [-2, 2] / 8  integers in [-2, 2]
    eighths   multiples of 1/8           integers in [-2, 2]  the same                 the same
    generic   multiples of 2^-10, < 16   randn, fp32          0.1 randn, fp32          randn, fp32   (fp32 kernels only)

In the generic family fl32(base + fl32(off + bias)) and the weight products hh hw are exact, so kernel and float64
agree on every floor and validity decision and only the arithmetic of the values is rounded.

TERMS, the longest chain of fp32 roundings that leads to an entry (csrc/dcn.hip):
    out   4 + 144      col: four corner products added in a chain (sample16 / sample16f; the weights hh hw are exact
                       here); then 9 taps x 16 channels of the group through the MFMA / fmaf accumulator (the other
                       48 channels of a bf16 tap multiply zeros of the block-diagonal weight)
    dcol  16           the 16 output channels of the group (MFMA over 64 with 48 zeros; 16 fmaf in k_bwd_f32)
    doff  16 + 16 + 4 + 2   dcol; sv = sum over the group's 16 channels of dcol v; the four corners into gh / gw; the
                       four groups by two xor shuffles
    dx    16 + 1 + hits + 4 + 1   dcol; the product weight x dcol (rounded on the atomic paths, exact in the S_k
                       MFMA); one addition per (pixel, tap, corner) contribution that reaches the input pixel, in the
                       window accumulator, the LDS atomics or the global atomics (hits, from the reference); at most
                       4 window slabs in k_gather_dx; dx[e] += s. (The issue's count had no term for the last one.)
    dW    4 + B H W    col; 64 pixels per tile in the MFMA / fmaf accumulator, then one slab per tile (k_slab_reduce
                       sums them in double and rounds once, inside the + 8)
    dob   38 + B H W   doff; 16 pixels by shuffles and 4 waves per tile (64 in a loop for fp32), one slab per tile
"""
import collections
import functools
import zlib

import torch

from oracle.dcn import deform_conv2d

U = 2.0 ** -24
C, CG, KT, TE, WE = 64, 16, 9, 8, 12
RPC_ERR_ARG, RPC_ERR_WORKSPACE, RPC_ERR_UNSUPPORTED = 1, 2, 3

DYADIC = ("halves", "eighths")
GRID = {"halves": 0.5, "eighths": 0.125, "generic": 2.0 ** -10}
XMAX = {"halves": 8, "eighths": 2}
# the smallest shapes at which each mechanism exists: one tile (every window edge outside the image); the batch
# index with one tile per frame; TY = 1 / TX = 1 with interior tile edges on the other axis; 2 x 3 tiles (a tile with
# neighbours on both sides, frames that differ)
SHAPES = [(1, 8, 8), (3, 8, 8), (1, 8, 32), (1, 32, 8), (2, 16, 24)]
PROBE_SHAPES = [(1, 8, 8), (2, 16, 24)]
GENERIC_SHAPES = [(1, 8, 8), (2, 16, 24)]
RANDOM = ("random",)
CLASS_FLOOR = 20

Case = collections.namedtuple("Case", "family shape pattern x off ob W gout")
Ref = collections.namedtuple("Ref", "out dx doff dob dW m_out m_dx m_doff m_dob m_dW hits")


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def to_rows(nchw):
    return nchw.permute(0, 2, 3, 1).reshape(-1, nchw.shape[1]).contiguous()


def to_nchw(rows, shape):
    B, H, W = shape
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def bf16_round(t):
    return t.float().to(torch.bfloat16).double()


def is_bf16(t):
    return bool((bf16_round(t) == t).all())


def is_f32(t):
    return bool((t.float().double() == t).all())


# ------------------------------------------------------------------ offset patterns
SHIFT_STEPS = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0)     # 1 is the window's design limit; 3/2 and 2 split a sample's corners
EIGHTH_STEPS = (0.125, 0.875, 1.125, 1.875, 2.125)   # either side of the same edges, on the eighths grid only
EDGES = ("-1", "-1/2", "n-1", "n-1/2", "n")


def edge_value(name, n):
    return {"-1": -1.0, "-1/2": -0.5, "n-1": n - 1.0, "n-1/2": n - 0.5, "n": float(n)}[name]


def probes(family):
    """one offset applied to all taps of all pixels (shift, far), per pixel row / column (row, col) or per pixel and
    tap (converge)"""
    out = [("zero",)]
    steps = SHIFT_STEPS + (EIGHTH_STEPS if family == "eighths" else ())
    for a in steps:
        for s in (1.0, -1.0):
            out += [("shift", s * a, 0.0), ("shift", 0.0, s * a), ("shift", s * a, s * a), ("shift", s * a, -s * a)]
    out += [("row", e) for e in EDGES] + [("col", e) for e in EDGES]
    out += [("far", 30.0, 30.0), ("far", -30.0, -30.0), ("far", 30.0, 0.0), ("far", 0.0, -30.0)]
    out += [("converge", "corner"), ("converge", "interior")]
    return out


def dyadic_cases():
    """(family, shape, pattern): the random draw at every shape, every probe at PROBE_SHAPES"""
    out = [(f, s, RANDOM) for f in DYADIC for s in SHAPES]
    out += [(f, s, p) for f in DYADIC for s in PROBE_SHAPES for p in probes(f)]
    return out


def case_id(c):
    f, s, p = c
    return f"{f}-{'x'.join(map(str, s))}-" + "_".join(str(v) for v in p)


def converge_pixel(which, shape):
    _, H, W = shape
    return (0, 0) if which == "corner" else (H // 2 + 1, W // 2 - 2)


def _total_offsets(family, shape, pattern, g):
    """the offsets the kernel samples with (offset image + bias) [B, 18, H, W], on the family's grid"""
    B, H, W = shape
    q = GRID[family]
    ys = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    ti = (torch.arange(KT) // 3).double().view(1, KT, 1, 1)
    tj = (torch.arange(KT) % 3).double().view(1, KT, 1, 1)
    dy = torch.zeros((B, KT, H, W), dtype=torch.float64)
    dx = torch.zeros((B, KT, H, W), dtype=torch.float64)
    kind = pattern[0]
    if kind == "random":
        # uniform within +-3, one in ten within +-30 (+-15 for the generic family, whose offsets stay below 16)
        n, far = int(round(3 / q)), int(round((15 if family == "generic" else 30) / q))
        t = torch.randint(-n, n + 1, (B, 2 * KT, H, W), generator=g).double() * q
        f = torch.randint(-far, far + 1, (B, 2 * KT, H, W), generator=g).double() * q
        pick = torch.rand((B, 2 * KT, H, W), generator=g) < 0.1
        return torch.where(pick, f, t)
    if kind in ("shift", "far"):
        dy, dx = dy + pattern[1], dx + pattern[2]
    elif kind == "row":      # every sample of tap row 0 exactly on the edge value, tap rows 1, 2 one and two below
        dy = dy + (edge_value(pattern[1], H) - (ys - 1))
    elif kind == "col":
        dx = dx + (edge_value(pattern[1], W) - (xs - 1))
    elif kind == "converge":  # every tap of every pixel samples input pixel (cy, cx) of its own frame
        cy, cx = converge_pixel(pattern[1], shape)
        dy = dy + (cy - (ys - 1 + ti))
        dx = dx + (cx - (xs - 1 + tj))
    elif kind != "zero":
        raise ValueError(pattern)
    return torch.stack([dy, dx], 2).reshape(B, 2 * KT, H, W)


@functools.lru_cache(maxsize=64)
def make_case(family, shape, pattern):
    """seeded inputs: x, dOut [B, 64, H, W], the offset image off [B, 18, H, W] and the offset bias ob [18] (the
    kernel samples with off + ob), W [64, 16, 3, 3]; float64 holding values of the kernels' own formats"""
    B, H, W = shape
    g = gen("dcn", family, shape, pattern)
    q = GRID[family]
    if family == "generic":
        x = torch.randn((B, C, H, W), generator=g).double()
        Wt = (torch.randn((C, CG, 3, 3), generator=g) * 0.1).double()
        gout = torch.randn((B, C, H, W), generator=g).double()
        nb = int(round(0.5 / q))
    else:
        m = XMAX[family]
        x = torch.randint(-m, m + 1, (B, C, H, W), generator=g).double()
        Wt = torch.randint(-2, 3, (C, CG, 3, 3), generator=g).double() / 8
        gout = torch.randint(-2, 3, (B, C, H, W), generator=g).double()
        nb = int(round(1 / q))
    ob = torch.randint(-nb, nb + 1, (2 * KT,), generator=g).double() * q
    total = _total_offsets(family, shape, pattern, g)
    off = total - ob.view(1, -1, 1, 1)
    # what the family relies on, by round trip: the images are bf16 (fp32 for generic) numbers, the bias is fp32, and
    # the kernel's fl32(off + ob) and fl32(base + that) are the exact sums
    img = is_f32 if family == "generic" else is_bf16
    assert img(x) and img(Wt) and img(gout) and img(off), (family, shape, pattern)
    assert is_f32(ob) and is_f32(off + ob.view(1, -1, 1, 1)) and bool((off + ob.view(1, -1, 1, 1) == total).all())
    base = torch.arange(-1, max(H, W) + 2, dtype=torch.float64).view(-1, 1, 1, 1, 1)
    assert is_f32(base + total)
    assert float(total.abs().max()) < (16 if family == "generic" else 32)
    return Case(family, shape, pattern, x, off, ob, Wt, gout)


def total_offsets(case):
    return case.off + case.ob.view(1, -1, 1, 1)


# ------------------------------------------------------------------ the operation, stated explicitly
def _corners(hl, wl, lh, lw):
    """(dy, dx, bilinear weight, d weight / d ph, d weight / d pw) of the four corners: mmcv
    deformable_im2col_bilinear and get_coordinate_weight (the weight's derivative, one-sided on an integer position)"""
    hh, hw = 1 - lh, 1 - lw
    return ((0, 0, hh * hw, -hw, -hh), (0, 1, hh * lw, -lw, hh), (1, 0, lh * hw, hw, -lh), (1, 1, lh * lw, lw, lh))


def explicit(x, offt, Wt, gout, absolute=False, keep=False):
    """The DCN forward and all its gradients as the kernels compute them, tap by tap and corner by corner, float64:
    col -> out; dcol = W_k^T dOut -> dW, dx (scatter of weight x dcol) and doff (get_coordinate_weight x dcol x the
    corner values). absolute: the same sums over |x|, |W|, |dOut| and |coordinate weight| = sum |a| |w| of every
    entry. keep: also the per-tap col, dcol and bilinear weights. hits [B, H W]: contributions per input pixel."""
    B, _, H, W = x.shape
    if absolute:
        x, Wt, gout = x.abs(), Wt.abs(), gout.abs()
    ys = torch.arange(H, dtype=x.dtype).view(1, H, 1)
    xs = torch.arange(W, dtype=x.dtype).view(1, 1, W)
    flat = x.reshape(B, C, H * W)
    Wg = Wt.reshape(4, CG, CG, KT)                      # [group][co][ci][tap]
    gg = gout.reshape(B, 4, CG, H, W)
    out = x.new_zeros((B, 4, CG, H, W))
    dx = x.new_zeros((B, C, H * W))
    doff = x.new_zeros((B, 2 * KT, H, W))
    dW = x.new_zeros((4, CG, CG, KT))
    hits = x.new_zeros((B, H * W))
    kept = {"col": [], "dcol": [], "wgt": []}
    for k in range(KT):
        ph = ys - 1 + k // 3 + offt[:, 2 * k]
        pw = xs - 1 + k % 3 + offt[:, 2 * k + 1]
        valid = (ph > -1) & (pw > -1) & (ph < H) & (pw < W)
        hl, wl = torch.floor(ph), torch.floor(pw)
        wk = Wg[..., k]
        dcol = torch.einsum("goc,bgohw->bgchw", wk, gg).reshape(B, C, H, W)
        col = x.new_zeros((B, C, H, W))
        gh, gw = x.new_zeros((B, H, W)), x.new_zeros((B, H, W))
        for dy, dxx, wgt, ch, cw in _corners(hl, wl, ph - hl, pw - wl):
            cy, cx = hl + dy, wl + dxx
            ok = (valid & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)).to(x.dtype)
            idx = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).long().view(B, 1, H * W)
            v = flat.gather(2, idx.expand(B, C, H * W)).view(B, C, H, W)
            wo = (wgt * ok).unsqueeze(1)
            col = col + wo * v
            sv = (dcol * v).sum(1)
            gh = gh + (ch.abs() if absolute else ch) * ok * sv
            gw = gw + (cw.abs() if absolute else cw) * ok * sv
            dx.scatter_add_(2, idx.expand(B, C, H * W), (wo * dcol).reshape(B, C, H * W))
            hits.scatter_add_(1, idx.view(B, H * W), ok.reshape(B, H * W))
            if keep:
                kept["wgt"].append(wgt * ok)
        colg = col.view(B, 4, CG, H, W)
        out = out + torch.einsum("goc,bgchw->bgohw", wk, colg)
        dW[..., k] = torch.einsum("bgohw,bgchw->goc", gg, colg)
        doff[:, 2 * k], doff[:, 2 * k + 1] = gh, gw
        if keep:
            kept["col"].append(col)
            kept["dcol"].append(dcol)
    res = {"out": out.reshape(B, C, H, W), "dx": dx.view(B, C, H, W), "doff": doff, "dob": doff.sum((0, 2, 3)),
           "dW": dW.reshape(C, CG, 3, 3), "hits": hits.view(B, H, W)}
    res.update(kept)
    return res


def autograd_ref(case):
    """out, dx, doff, dob, dW of oracle.dcn.deform_conv2d and torch autograd"""
    xr = case.x.clone().requires_grad_(True)
    offr = total_offsets(case).clone().requires_grad_(True)
    Wr = case.W.clone().requires_grad_(True)
    out = deform_conv2d(xr, offr, Wr, groups=4)
    (out * case.gout).sum().backward()
    return {"out": out.detach(), "dx": xr.grad, "doff": offr.grad, "dob": offr.grad.sum((0, 2, 3)), "dW": Wr.grad}


# units of the families' grids: x 1, W 1/8, dOut 1, offsets q -> bilinear weights q^2, coordinate weights q
def _units(family):
    q = GRID[family]
    return {"out": q * q / 8, "dx": q * q / 8, "doff": q / 8, "dob": q / 8, "dW": q * q}


@functools.lru_cache(maxsize=64)
def reference(family, shape, pattern):
    """float64 reference and magnitudes of a case (cached: the reference is the cost of these tests). For the dyadic
    families it asserts what makes the test sharp: col, dcol and the bilinear weights of every tap are bf16 numbers,
    every output is an fp32 number and every sum |a| |w| (for dob: sum |doff|) is below 2^24 units of its grid."""
    case = make_case(family, shape, pattern)
    offt = total_offsets(case)
    a = autograd_ref(case)
    m = explicit(case.x, offt, case.W, case.gout, absolute=True)
    if family in DYADIC:
        e = explicit(case.x, offt, case.W, case.gout, keep=True)
        for name in ("col", "dcol", "wgt"):
            for k, t in enumerate(e[name]):
                assert is_bf16(t), (family, shape, pattern, name, k)
        for name, unit in _units(family).items():
            assert is_f32(a[name]), (family, shape, pattern, name)
            assert bool((a[name] == e[name]).all()), (family, shape, pattern, name)
            # dob sums the (exact) doff values: its partial sums in any order stay below sum |doff|, which is far
            # smaller than the sum |a| |w| of its bound when every sample is valid (the zero probe)
            top = a["doff"].abs().sum((0, 2, 3)) if name == "dob" else m[name]
            assert float(top.max()) / unit < 2.0 ** 24, (family, shape, pattern, name, float(top.max()) / unit)
    return Ref(a["out"], a["dx"], a["doff"], a["dob"], a["dW"], m["out"], m["dx"], m["doff"], m["dob"], m["dW"],
               m["hits"])


def terms(name, shape, hits=None):
    B, H, W = shape
    if name == "out":
        return 4 + 144
    if name == "doff":
        return 16 + 16 + 4 + 2
    if name == "dx":
        return 16 + 1 + hits.unsqueeze(1) + 4 + 1
    if name == "dW":
        return 4 + B * H * W
    if name == "dob":
        return 16 + 16 + 4 + 2 + B * H * W
    raise ValueError(name)


def bound(name, ref, shape):
    """b = (terms + 8) u sum |a| |w| of output name, a tensor of the output's shape"""
    t = terms(name, shape, ref.hits)
    return (t + 8) * U * getattr(ref, "m_" + name)


def bf16_interval(ref, b):
    """[bf16(ref - b), bf16(ref + b)]: the bf16 numbers a correctly rounded store of a value within b of ref can
    give. Not b + 2^-9 |ref|: that would hide a one-unit error at |out| = 37."""
    return bf16_round(ref - b), bf16_round(ref + b)


def bad_entries(got, ref, b, bf16):
    """mask of the entries outside the criterion (a NaN is outside)"""
    if bf16:
        lo, hi = bf16_interval(ref, b)
        return ~((got >= lo) & (got <= hi))
    return ~((got - ref).abs() <= b)


# ------------------------------------------------------------------ sample classes
CLASSES = ("invalid", "on_edge", "valid_integer", "valid_partial", "window_in", "window_out", "window_mixed")


def classify(offt, shape):
    """sample counts of a case per class: invalid; exactly on -1 / H / W (invalid, one step from valid); valid on an
    integer row or column (one-sided coordinate weights); valid with 1..3 corners outside the image; valid with all
    its in-image corners inside the 12 x 12 window of its tile, all outside it, and some of each"""
    B, H, W = shape
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    y0, x0 = torch.floor(ys / TE) * TE - 2, torch.floor(xs / TE) * TE - 2
    n = dict.fromkeys(CLASSES, 0)
    for k in range(KT):
        ph = ys - 1 + k // 3 + offt[:, 2 * k]
        pw = xs - 1 + k % 3 + offt[:, 2 * k + 1]
        valid = (ph > -1) & (pw > -1) & (ph < H) & (pw < W)
        hl, wl = torch.floor(ph), torch.floor(pw)
        inimg = torch.zeros((B, H, W))
        inwin = torch.zeros((B, H, W))
        for dy in (0, 1):
            for dx in (0, 1):
                cy, cx = hl + dy, wl + dx
                ok = (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
                win = (cy >= y0) & (cy < y0 + WE) & (cx >= x0) & (cx < x0 + WE)
                inimg += ok
                inwin += ok & win
        n["invalid"] += int((~valid).sum())
        n["on_edge"] += int(((ph == -1) | (ph == H) | (pw == -1) | (pw == W)).sum())
        n["valid_integer"] += int((valid & ((ph == hl) | (pw == wl))).sum())
        n["valid_partial"] += int((valid & (inimg < 4)).sum())
        n["window_in"] += int((valid & (inwin == inimg)).sum())
        n["window_out"] += int((valid & (inwin == 0)).sum())
        n["window_mixed"] += int((valid & (inwin > 0) & (inwin < inimg)).sum())
    return n
