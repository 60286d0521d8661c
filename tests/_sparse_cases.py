"""Shared inputs and float64 references for the sparse rulebook and the fp32 and 16-bit sparse-conv kernel tests (no
GPU code).

Voxel sets on tiny grids that hold the places where a rulebook goes wrong (faces and corners of the volume, the
seam between two frames of the linear grid, a voxel with no neighbour), rulebooks by brute force over a Python
dict from coordinate to row (nothing is linearised, so nothing can wrap), and float64 restatements of the sparse
convolution's forward, data gradient and weight gradient as include/rpc_hip.h specifies them. Every reference
value comes with the sum of the magnitudes of its terms, S: fp32 summation in any order stays within
(terms + c) * 2^-24 * S of the exact sum, which is the bound the kernel tests hold the HIP kernels to.
"""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # fp32 unit roundoff
TILE = 64               # rows per GEMM tile = rows per BatchNorm partial row (rpc_spconv_gemm_blocks)

GRIDS = [(2, 5, 7, 6), (3, 4, 9, 8)]     # (B, D, H, W): odd and even extents
# (ksize, stride, pad) of the strided convolutions the encoders use
GEOMS = [((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)), ((3, 1, 1), (2, 1, 1), (0, 0, 0))]


# ------------------------------------------------------------------ voxel sets
def corner_case_coors(shape, n, seed):
    """n unique int32 (b, z, y, x) rows in shuffled order: the 8 corners of frame 0 (the last cell of frame 0
    among them), the first cell of frame 1, one full line along each axis (frame 1), one voxel of frame 0 with
    no 3x3x3 neighbour, random fill."""
    B, D, H, W = shape
    assert B >= 2 and D >= 4 and H >= 5 and W >= 5
    must = [(0, z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
    must.append((1, 0, 0, 0))
    must += [(1, D // 2, H // 2, x) for x in range(W)]
    must += [(1, D // 2, y, 1) for y in range(H)]
    must += [(1, z, H - 2, W - 2) for z in range(D)]
    iso = (0, D // 2, H // 2, W // 2)
    must.append(iso)
    must = list(dict.fromkeys(must))
    near = {(0, iso[1] + a, iso[2] + b, iso[3] + c) for a, b, c in itertools.product((-1, 0, 1), repeat=3)}
    assert not (near & set(must)) - {iso}
    assert len(must) <= n
    rng = np.random.default_rng(seed)
    taken = near | set(must)
    free = [c for c in itertools.product(range(B), range(D), range(H), range(W)) if c not in taken]
    pick = rng.choice(len(free), n - len(must), replace=False)
    rows = must + [free[i] for i in pick]
    out = np.asarray(rows, np.int32)[rng.permutation(n)]
    assert len({tuple(c) for c in out.tolist()}) == n
    return out


def small_coors(shape, n):
    """n = 1: the far corner of the last frame; n = 2: the last cell of frame 0 and the first cell of frame 1."""
    B, D, H, W = shape
    if n == 1:
        return np.asarray([(B - 1, D - 1, H - 1, W - 1)], np.int32)
    assert n == 2
    return np.asarray([(0, D - 1, H - 1, W - 1), (1, 0, 0, 0)], np.int32)


def coors_for(shape, n, seed=0):
    return small_coors(shape, n) if n <= 2 else corner_case_coors(shape, n, seed)


def out_shape(shape, ksize, stride, pad):
    return (shape[0],) + tuple((shape[1 + a] + 2 * pad[a] - ksize[a]) // stride[a] + 1 for a in range(3))


# ------------------------------------------------------------------ brute-force rulebooks
def _offsets(ksize):
    """[(k, (kz, ky, kx))] with k = (kz * kh + ky) * kw + kx"""
    kd, kh, kw = ksize
    return [((kz * kh + ky) * kw + kx, (kz, ky, kx)) for kz in range(kd) for ky in range(kh) for kx in range(kw)]


def subm_rulebook(coors, ksize=(3, 3, 3)):
    """nbr[r, k] = row at coors[r] + (k - centre), or -1"""
    row = {tuple(c): r for r, c in enumerate(coors.tolist())}
    offs = _offsets(ksize)
    nbr = np.full((len(coors), len(offs)), -1, np.int32)
    for r, (b, z, y, x) in enumerate(coors.tolist()):
        for k, (kz, ky, kx) in offs:
            nbr[r, k] = row.get((b, z + kz - ksize[0] // 2, y + ky - ksize[1] // 2, x + kx - ksize[2] // 2), -1)
    return nbr


def strided_rulebook(coors, shape_in, ksize, stride, pad):
    """(coors_out, nbr_out [n_out, K], nbr_in [n_in, K]): input c reaches output o = (c + pad - k) / stride through
    offset k where that is a whole, in-range coordinate; output rows are numbered in the order of their first
    candidate, i.e. ascending r * K + k."""
    oshape = out_shape(shape_in, ksize, stride, pad)
    offs = _offsets(ksize)
    orow, coors_out = {}, []
    nbr_in = np.full((len(coors), len(offs)), -1, np.int32)
    for r, c in enumerate(coors.tolist()):
        for k, kk in sorted(offs):
            n = [c[1 + a] + pad[a] - kk[a] for a in range(3)]
            if any(v < 0 or v % s for v, s in zip(n, stride)):
                continue
            o = tuple(v // s for v, s in zip(n, stride))
            if any(v >= m for v, m in zip(o, oshape[1:])):
                continue
            key = (c[0],) + o
            if key not in orow:
                orow[key] = len(coors_out)
                coors_out.append(key)
            nbr_in[r, k] = orow[key]
    nbr_out = np.full((len(coors_out), len(offs)), -1, np.int32)
    for r, k in zip(*np.nonzero(nbr_in >= 0)):
        assert nbr_out[nbr_in[r, k], k] == -1
        nbr_out[nbr_in[r, k], k] = r
    return np.asarray(coors_out, np.int32).reshape(-1, 4), nbr_out, nbr_in


def pair_set(nbr, coors_in, coors_out):
    """neighbour map nbr[o, k] = i as the set of (k, in coordinate, out coordinate)"""
    o, k = np.nonzero(nbr >= 0)
    ci, co = coors_in[nbr[o, k]].tolist(), coors_out[o].tolist()
    return {(int(kk), tuple(a), tuple(b)) for kk, a, b in zip(k, ci, co)}


# ------------------------------------------------------------------ float64 references
def _d(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def act_ref(x, bn):
    """(A, M): A = relu((x - mean) * scale + beta) with bn = scale, beta, mean, invstd [4C], or x itself (bn None);
    M = |x - mean| * |scale| + |beta|, the magnitude the transform's roundings are relative to (None for bn None)."""
    x = _d(x)
    if bn is None:
        return x, None
    sc, be, mu = _d(bn).view(4, -1)[:3]
    return torch.relu((x - mu) * sc + be), (x - mu).abs() * sc.abs() + be.abs()


def bnbwd_ref(dy, z, bnb):
    """(dz, mag): dz = gi * (dy - m1 - xhat * m2), xhat = (z - mean) * invstd, bnb = gi, m1, m2, mean, invstd [5C];
    mag = |gi| * (|dy| + |m1| + |xhat| * |m2|), the uncancelled magnitude"""
    dy, z = _d(dy), _d(z)
    gi, m1, m2, mu, is_ = _d(bnb).view(5, -1)
    xh = (z - mu) * is_
    return gi * (dy - m1 - xh * m2), gi.abs() * (dy.abs() + m1.abs() + xh.abs() * m2.abs())


def conv_ref(x, nbr, W, in_bn=None):
    """z[r] = sum_k A(x[nbr[r, k]]) . W[k]; returns (z, S, T): S = sum |A| |W| per element, T = sum M |W| (the
    on-load transform's magnitude, zeros without in_bn)."""
    A, M = act_ref(x, in_bn)
    W = _d(W)
    nbr = torch.as_tensor(nbr).long()
    n, K = nbr.shape
    z = torch.zeros((n, W.shape[2]), dtype=torch.float64)
    S, T = torch.zeros_like(z), torch.zeros_like(z)
    for k in range(K):
        ok = nbr[:, k] >= 0
        if ok.any():
            i = nbr[ok, k]
            z[ok] += A[i] @ W[k]
            S[ok] += A[i].abs() @ W[k].abs()
            if M is not None:
                T[ok] += M[i] @ W[k].abs()
    return z, S, T


def dgrad_ref(dy, z, bnb, mp, rev, W, prev_z=None, prev_bn=None):
    """din[i] = sum_k dz[map[i, k']] . W[k]^T, k' = K-1-k if rev else k; with prev_z / prev_bn (scale, beta, mean,
    invstd) the previous layer's ReLU mask is applied. Returns (din, S, xhat_prev or None)."""
    dz, mag = bnbwd_ref(dy, z, bnb)
    W = _d(W)
    mp = torch.as_tensor(mp).long()
    n, K = mp.shape
    din = torch.zeros((n, W.shape[1]), dtype=torch.float64)
    S = torch.zeros_like(din)
    for k in range(K):
        col = mp[:, K - 1 - k if rev else k]
        ok = col >= 0
        if ok.any():
            din[ok] += dz[col[ok]] @ W[k].T
            S[ok] += mag[col[ok]] @ W[k].abs().T
    if prev_z is None:
        return din, S, None
    sc, be, mu, is_ = _d(prev_bn).view(4, -1)
    pz = _d(prev_z)
    m = ((pz - mu) * sc + be > 0).double()
    return din * m, S * m, (pz - mu) * is_


def wgrad_ref(x, in_bn, nbr, dy, z, bnb):
    """dW[k] = sum_r A(x[nbr[r, k]])^T dz[r]; returns (dW, S, T) as conv_ref does"""
    A, M = act_ref(x, in_bn)
    dz, mag = bnbwd_ref(dy, z, bnb)
    nbr = torch.as_tensor(nbr).long()
    K = nbr.shape[1]
    dW = torch.zeros((K, A.shape[1], dz.shape[1]), dtype=torch.float64)
    S, T = torch.zeros_like(dW), torch.zeros_like(dW)
    for k in range(K):
        ok = nbr[:, k] >= 0
        if ok.any():
            i = nbr[ok, k]
            dW[k] = A[i].T @ dz[ok]
            S[k] = A[i].abs().T @ mag[ok]
            if M is not None:
                T[k] = M[i].T @ mag[ok]
    return dW, S, T


def tile_sums(v):
    """column sums of v [n, C] per TILE rows in float64: (sums [tiles, C], sums of |.|)"""
    v = _d(v)
    n, C = v.shape
    t = (n + TILE - 1) // TILE
    p = torch.zeros((t * TILE, C), dtype=torch.float64)
    p[:n] = v
    p = p.view(t, TILE, C)
    return p.sum(1), p.abs().sum(1)


def relu_mask_ref(z, bn):
    sc, be, mu = _d(bn).view(4, -1)[:3]
    return (_d(z) - mu) * sc + be > 0


def decisive_z(n, bn, gen, margin=1e-3):
    """fp32 z [n, C] whose pre-activations (z - mean) * scale + beta all lie at least margin from 0 (redrawn until
    they do): the fp32 kernel's rounding (<= 2 * 2^-24 * M) cannot move one across, so its ReLU decision is
    float64's."""
    C = bn.numel() // 4
    sc, be, mu = bn.double().view(4, C)[:3]
    z = torch.randn((n, C), generator=gen) * 2
    for _ in range(100):
        bad = ((z.double() - mu) * sc + be).abs() < margin
        if not bad.any():
            return z
        z[bad] = (torch.randn((n, C), generator=gen) * 2)[bad]
    raise AssertionError("decisive_z did not converge")


# ------------------------------------------------------------------ an independent dense operation
def dense_conv_ref(x, coors, shape, W, ksize, stride, pad):
    """float64 torch conv3d of the densified rows: (out [B, CO, D', H', W'], S = conv3d(|x|, |W|))"""
    x, W = _d(x), _d(W)
    B, D, H, Wd = shape
    c = torch.as_tensor(np.asarray(coors)).long()
    dense = torch.zeros((B, D, H, Wd, x.shape[1]), dtype=torch.float64)
    dense[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = x
    dense = dense.permute(0, 4, 1, 2, 3)
    w = W.view(ksize[0], ksize[1], ksize[2], W.shape[1], W.shape[2]).permute(4, 3, 0, 1, 2)
    return (F.conv3d(dense, w, stride=stride, padding=pad),
            F.conv3d(dense.abs(), w.abs(), stride=stride, padding=pad))


def read_sites(dense, coors):
    """rows [n, C] of a [B, C, D, H, W] image at coors"""
    c = torch.as_tensor(np.asarray(coors)).long()
    return dense[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


# ------------------------------------------------------------------ synthetic maps and parameters for the kernel tests
def random_map(n_out, n_in, K, seed, density=0.3):
    """[n_out, K] int32 indices into n_in rows at the given density, with: offset 1 used by nobody, rows 64..127 with
    no neighbour at all (n_out > 127), the last offset used by row 63 only (n_out > 63), and row 0 never empty."""
    g = torch.Generator().manual_seed(seed)
    nbr = torch.randint(0, n_in, (n_out, K), generator=g, dtype=torch.int32)
    nbr[torch.rand((n_out, K), generator=g) > density] = -1
    nbr[:, 1] = -1
    nbr[0, 0] = n_in // 2
    if n_out > 127:
        nbr[64:128] = -1
    if n_out > 63:
        nbr[:, K - 1] = -1
        nbr[63, K - 1] = n_in - 1
    return nbr


def bn_vec(c, gen):
    """scale (either sign), beta, mean, invstd [4c]"""
    sign = torch.where(torch.rand(c, generator=gen) < 0.25, -1.0, 1.0)
    return torch.cat([(torch.rand(c, generator=gen) + 0.5) * sign, torch.randn(c, generator=gen) * 0.3,
                      torch.randn(c, generator=gen) * 0.2, torch.rand(c, generator=gen) + 0.5])


def bnb_vec(c, gen):
    """gi, m1, m2, mean, invstd [5c]"""
    return torch.cat([torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.3,
                      torch.randn(c, generator=gen) * 0.3, torch.randn(c, generator=gen) * 0.2,
                      torch.rand(c, generator=gen) + 0.5])


# ------------------------------------------------------------------ 16-bit operands: the perf mode's GEMM family
# Rows and weights drawn on the 16-bit grid are read back unchanged by the float64 references below, every product of
# two of them is exact in fp32, and the weight-tile prep rounds nothing: what is left is the fp32 accumulation.
H16 = (torch.bfloat16, torch.float16)      # indexed by RPC_H16_BF16, RPC_H16_F16


def r8(c):
    return (c + 7) // 8 * 8


def r16(c):
    return (c + 15) // 16 * 16


def r32(c):
    return (c + 31) // 32 * 32


def h16_rows(n, c, gen, fmt, scale=1.0):
    """operand rows [n, round8(c)] in H16[fmt]: randn * scale rounded to the format, padding columns zero (the
    producers' contract: the GEMM reads those columns)"""
    h = torch.zeros((n, r8(c)), dtype=H16[fmt])
    h[:, :c] = (torch.randn((n, c), generator=gen) * scale).to(H16[fmt])
    return h


def h16_weights(K, ci, co, gen, fmt, scale=0.1):
    """fp32 W [K, ci, co] whose every value lies on the grid of H16[fmt]"""
    return (torch.randn((K, ci, co), generator=gen) * scale).to(H16[fmt]).float()


def sat_f16(x):
    """fp32 values as the fp16 producers see them: finite ones beyond +-65504 become +-65504, inf / NaN stay"""
    x = torch.as_tensor(x).float()
    big = torch.isfinite(x) & (x.abs() > 65504.0)
    return torch.where(big, torch.copysign(torch.full_like(x, 65504.0), x), x)


def to_h16(x, fmt):
    """fp32 -> H16[fmt] as the kernels round: to nearest even, fp16 saturated first"""
    x = torch.as_tensor(x).float()
    return (sat_f16(x) if fmt else x).to(H16[fmt])


def weight_tiles_ref(W, dgrad, fmt):
    """The layout include/rpc_hip.h states for rpc_spconv_prep_weight_bf16: W [K, ci, co] -> forward tiles
    [K, round16(co), round32(ci)] (tile[k, n, c] = W[k, c, n]), data-gradient tiles [K, round16(ci), round32(co)]
    (tile[k, n, c] = W[k, n, c]), zero padded, in H16[fmt]"""
    W = torch.as_tensor(W).float()
    B = W if dgrad else W.transpose(1, 2)
    t = torch.zeros((W.shape[0], r16(B.shape[1]), r32(B.shape[2])), dtype=H16[fmt])
    t[:, :B.shape[1], :B.shape[2]] = to_h16(B, fmt)
    return t


def gather_gemm_ref(a, mp, rev, B):
    """out[r] = sum_k a[mp[r, k'], :kg] . B[k], k' = K-1-k if rev else k, for ready rows a (any dtype, at least kg
    columns) and B [K, kg, ng]; returns (out, S), S = sum |a| |B| per element. One contraction over the gathered
    rows [n, K, kg] (a missing neighbour gathers zeros), not conv_ref's loop over offsets."""
    B = _d(B)
    K, kg, _ = B.shape
    a = _d(a)[:, :kg]
    mp = torch.as_tensor(mp).long()
    assert mp.shape[1] == K
    if rev:
        mp = mp.flip(1)
    G = a[mp.clamp_min(0)] * (mp >= 0).unsqueeze(-1)
    return torch.einsum("rkc,kcn->rn", G, B), torch.einsum("rkc,kcn->rn", G.abs(), B.abs())


def gather_wgrad_ref(h, nbr, dz):
    """dW[k] = sum_r h[nbr[r, k], :ci]^T dz[r, :co] for ready rows; h and dz carry exactly ci and co columns.
    Returns (dW, S, n_k): S = sum |h| |dz| per element, n_k [K] the number of rows that use offset k."""
    h, dz = _d(h), _d(dz)
    nbr = torch.as_tensor(nbr).long()
    ok = (nbr >= 0).double()
    G = h[nbr.clamp_min(0)] * ok.unsqueeze(-1)
    return (torch.einsum("rkc,rn->kcn", G, dz), torch.einsum("rkc,rn->kcn", G.abs(), dz.abs()),
            ok.sum(0).long())


def infer_ref(acc, fold, res=None):
    """The eval-mode epilogue y = relu(acc * scale + shift (+ res)) with fold = scale, shift [2C]; returns (y, M),
    M = |acc * scale| + |shift| + |res|, the magnitude its roundings are relative to"""
    acc = _d(acc)
    sc, sh = _d(fold).view(2, -1)
    pre, M = acc * sc + sh, (acc * sc).abs() + sh.abs()
    if res is not None:
        pre, M = pre + _d(res), M + _d(res).abs()
    return torch.relu(pre), M
