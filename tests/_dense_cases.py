"""Float64 references and case lists for the dense BEV engine's kernel tests (test_dense_cases_cpu.py pins them on
the CPU; test_gpu_dense_f32_kernels.py, test_gpu_dense_bn_passes.py and test_gpu_dense_igemm_maps.py use them).
No GPU import: images are [rows][C] tensors on the CPU, rows = NHWC pixels.

Maps as in csrc/dense_common.h. FS1 is S1 run with the data-gradient weights ([t][ci][co], taps flipped): the
data gradient of a stride-1 3x3 conv. R / S / O are the (B, H, W) of the GEMM-row, source and output images.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24                       # fp32 unit roundoff
S1, S2, D2, P1, U2, G2 = 0, 1, 2, 3, 4, 5
FS1 = 7                              # test-side name only: S1 with flipped data-gradient weights
MAP_NAMES = {S1: "S1", S2: "S2", D2: "D2", P1: "P1", U2: "U2", G2: "G2", FS1: "S1 flipped"}
ABI_MAP = {S1: S1, S2: S2, D2: D2, P1: P1, U2: U2, G2: G2, FS1: S1}
TAPS = {S1: 9, S2: 9, D2: 9, P1: 1, U2: 1, G2: 4, FS1: 9}
WTAPS = {S1: 9, S2: 9, P1: 1, U2: 4}
KIND = {S1: 0, S2: 0, D2: 0, FS1: 0, P1: 1, U2: 1, G2: 1}     # torch layer: 0 Conv2d, 1 ConvTranspose2d
BF16_SENTINEL = 0x7FC1               # a NaN pattern no rounding produces
RPC_ERR_ARG, RPC_ERR_WORKSPACE = 1, 2

# row images (B, H, W) around the fp32 engine's 64-row tile and the XCD remap (< 8 blocks, 17 blocks)
IMAGES_F32 = [(1, 1, 1), (1, 7, 9), (2, 4, 8), (1, 5, 13), (3, 5, 9), (2, 17, 32)]
# ... around the bf16 engine's 128-row tile
IMAGES_BF16 = [(1, 1, 1), (1, 9, 14), (2, 8, 8), (1, 3, 43), (3, 7, 13)]
# (full-resolution image, half-resolution image): odd and even extents of a stride-2 pair
S2_PAIRS = [((2, 9, 7), (2, 5, 4)), ((1, 8, 6), (1, 4, 3))]
CHANNELS_F32 = [(16, 64), (48, 128), (64, 192)]
CHANNELS_BF16 = [(64, 128), (128, 256), (64, 384)]
IMAGES_S1_BF16 = [(1, 16, 32), (2, 17, 33), (1, 9, 130), (3, 5, 7)]
CHANNELS_S1_BF16 = [(64, 128), (192, 128), (128, 256)]
# weight gradient: GEMM-row images of M = 1, 31, 32, 33, 1000 and one with more than 32 rows per chunk
WGRAD_IMAGES_F32 = [(1, 1, 1), (1, 1, 31), (1, 4, 8), (1, 3, 11), (2, 20, 25), (2, 48, 40)]
WGRAD_IMAGES_BF16 = [(1, 1, 1), (1, 1, 127), (1, 3, 43), (2, 20, 25)]
WGRAD_CHANNELS = [(64, 64), (64, 128), (128, 128)]
BN_CHANNELS = [8, 64, 128, 256, 384, 2048]
BN_ROWS = [0, 1, 7, 255, 257, 4099]


def bn_shapes():
    return [(c, m) for c in BN_CHANNELS for m in BN_ROWS if not (c == 2048 and m == max(BN_ROWS))]


def geometry(fmap, img):
    """(R, S, O) of a map whose GEMM-row image is img; S2 / G2 read the even-sized double image, D2 the half one"""
    B, H, W = img
    if fmap in (S1, FS1, P1):
        return img, img, img
    if fmap == S2:
        return img, (B, 2 * H, 2 * W), img
    if fmap == D2:
        return img, (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1), img
    if fmap == U2:
        return img, img, (B, 2 * H, 2 * W)
    if fmap == G2:
        return img, (B, 2 * H, 2 * W), img
    raise ValueError(fmap)


def conv_cases(fmap, images):
    """[(R, S, O)] for a map: the row images, and for S2 / D2 the odd and even stride-2 pairs"""
    out = [geometry(fmap, i) for i in images]
    if fmap == S2:
        out += [(half, full, half) for full, half in S2_PAIRS]
    if fmap == D2:
        out += [(full, half, full) for full, half in S2_PAIRS]
    return out


def npix(img):
    return img[0] * img[1] * img[2]


def _d(t):
    return t.detach().cpu().double()


def to_nchw(rows, img):
    B, H, W = img
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def to_rows(nchw):
    return nchw.permute(0, 2, 3, 1).reshape(-1, nchw.shape[1])


def layer_weight_shape(fmap, cin, cout):
    """torch weight shape of the layer behind a GEMM of cin -> cout channels on map fmap"""
    return {S1: (cout, cin, 3, 3), S2: (cout, cin, 3, 3), D2: (cin, cout, 3, 3), FS1: (cin, cout, 3, 3),
            P1: (cin, cout, 1, 1), U2: (cin, cout, 2, 2), G2: (cout, cin, 2, 2)}[fmap]


def _conv_op(fmap, x, W, R, S, O):
    xi = to_nchw(x, S)
    if fmap == S1:
        return to_rows(F.conv2d(xi, W, padding=1))
    if fmap == S2:
        return to_rows(F.conv2d(xi, W, stride=2, padding=1))
    if fmap == P1:
        return to_rows(F.conv_transpose2d(xi, W))
    if fmap == U2:
        return to_rows(F.conv_transpose2d(xi, W, stride=2))
    # data gradients by autograd: the layer is linear, so its input gradient does not depend on the input
    B, H, Wd = O
    if fmap in (D2, FS1):
        inp = torch.zeros((B, W.shape[1], H, Wd), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(inp, W, stride=2 if fmap == D2 else 1, padding=1)
    else:
        inp = torch.zeros((B, W.shape[0], H, Wd), dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose2d(inp, W, stride=2)
    assert tuple(y.shape) == tuple(xi.shape), (fmap, y.shape, xi.shape)
    y.backward(xi)
    return to_rows(inp.grad)


def conv_ref(fmap, x, W, kind, R, S, O):
    """x [S pixels][cin], W the torch weight of the layer (kind 0: Conv2d, 1: ConvTranspose2d) -> (ref, mag)
    [O pixels][cout] float64; mag is the same operation on |x|, |W| = sum |a| |w| per output element"""
    assert kind == KIND[fmap]
    x, W = _d(x), _d(W)
    return _conv_op(fmap, x, W, R, S, O), _conv_op(fmap, x.abs(), W.abs(), R, S, O)


def _wgrad_op(fmap, x, dz, wshape, R, S, O):
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    xi, gi = to_nchw(x, S), to_nchw(dz, O)
    if fmap == S1:
        y = F.conv2d(xi, w, padding=1)
    elif fmap == S2:
        y = F.conv2d(xi, w, stride=2, padding=1)
    elif fmap == P1:
        y = F.conv_transpose2d(xi, w)
    else:
        y = F.conv_transpose2d(xi, w, stride=2)
    assert tuple(y.shape) == tuple(gi.shape)
    y.backward(gi)
    return w.grad


def wgrad_ref(fmap, x, dz, kind, R, S, O):
    """x [S pixels][ci], dz [O pixels][co] -> (dW, mag) in the torch layout of the layer, float64"""
    assert kind == KIND[fmap]
    x, dz = _d(x), _d(dz)
    ci, co = x.shape[1], dz.shape[1]
    k = {S1: 3, S2: 3, P1: 1, U2: 2}[fmap]
    shape = (co, ci, k, k) if kind == 0 else (ci, co, k, k)
    return _wgrad_op(fmap, x, dz, shape, R, S, O), _wgrad_op(fmap, x.abs(), dz.abs(), shape, R, S, O)


def src_rows(fmap, R, S):
    """[M][T] int64: src_row<MAP> of csrc/dense_common.h, -1 where the tap has no source"""
    fmap = ABI_MAP[fmap]
    B, H, W = R
    T = TAPS[fmap]
    m = torch.arange(B * H * W)
    b, y, x = m // (H * W), (m % (H * W)) // W, m % W
    out = torch.full((B * H * W, T), -1, dtype=torch.int64)
    for t in range(T):
        ok = torch.ones_like(m, dtype=torch.bool)
        if fmap == S1:
            sy, sx = y + t // 3 - 1, x + t % 3 - 1
        elif fmap == S2:
            sy, sx = 2 * y + t // 3 - 1, 2 * x + t % 3 - 1
        elif fmap == D2:
            oy, ox = y + 1 - t // 3, x + 1 - t % 3
            ok = (oy >= 0) & (ox >= 0) & (oy % 2 == 0) & (ox % 2 == 0)
            sy, sx = oy // 2, ox // 2
        elif fmap == G2:
            sy, sx = 2 * y + (t >> 1), 2 * x + (t & 1)
        else:
            sy, sx = y, x
        ok = ok & (sy >= 0) & (sy < S[1]) & (sx >= 0) & (sx < S[2])
        out[:, t] = torch.where(ok, (b * S[1] + sy) * S[2] + sx, torch.full_like(m, -1))
    return out


def out_rows(R, O, par):
    """out_row<M_U2>: the output pixel of GEMM row m for parity par"""
    B, H, W = R
    m = torch.arange(B * H * W)
    b, y, x = m // (H * W), (m % (H * W)) // W, m % W
    return (b * O[1] + 2 * y + (par >> 1)) * O[2] + 2 * x + (par & 1)


def gemm_weights(fmap, W):
    """the kernel's weight operand [taps][cout][cin] of the layer weight W, as rpc_dense_wprep lays it out (a pure
    permutation; the wprep tests hold the kernels to it bit for bit)"""
    if fmap in (S1, S2):                       # fwd of Conv2d [co][ci][3][3] -> [t][co][ci]
        return W.reshape(W.shape[0], W.shape[1], 9).permute(2, 0, 1).contiguous()
    if fmap in (D2, FS1):                      # dgrad of Conv2d -> [td][ci][co], td flipped for stride 1
        w = W.reshape(W.shape[0], W.shape[1], 9).permute(2, 1, 0)
        return (w.flip(0) if fmap == FS1 else w).contiguous()
    if fmap in (P1, U2):                       # fwd of ConvTranspose2d [ci][co][k][k] -> [t][co][ci]
        T = W.shape[2] * W.shape[3]
        return W.reshape(W.shape[0], W.shape[1], T).permute(2, 1, 0).contiguous()
    return W.reshape(W.shape[0], W.shape[1], 4).permute(2, 0, 1).contiguous()     # G2: dgrad [t][ci][co]


def gather_conv(fmap, x, W, R, S, O):
    """the GEMM as the kernels state it: out[out_row(m)] = sum_t wt[t] @ x[src_row(m, t)], an explicit loop"""
    x = _d(x)
    wt = _d(gemm_weights(fmap, W))
    sr = src_rows(fmap, R, S)
    cout = wt.shape[1]
    out = torch.zeros((npix(O), cout), dtype=torch.float64)
    for par in range(4 if fmap == U2 else 1):
        orow = out_rows(R, O, par) if fmap == U2 else torch.arange(npix(R))
        for m in range(npix(R)):
            acc = torch.zeros(cout, dtype=torch.float64)
            for t in range(sr.shape[1]):
                if sr[m, t] >= 0:
                    acc += wt[par if fmap == U2 else t] @ x[sr[m, t]]
            out[orow[m]] = acc
    return out


def tap_counts(fmap, R, S):
    """rows whose tap t lies inside the source image, per weight-gradient tap"""
    if fmap == U2:
        return torch.full((4,), npix(R), dtype=torch.int64)
    return (src_rows(fmap, R, S) >= 0).sum(0)


def wgrad_bound_terms(fmap, kind, R, S, shape):
    """n_t broadcast to the torch weight layout [..][..][k][k]"""
    nt = tap_counts(fmap, R, S).double()
    k = shape[2]
    return nt.view(1, 1, k, k)


# ------------------------------------------------------------------ pitched buffers inside a sentinel fill
def sentinel_buffer(rows, pitch, dtype):
    if dtype == torch.bfloat16:
        return torch.full((rows, pitch), BF16_SENTINEL, dtype=torch.int16).view(torch.bfloat16)
    return torch.full((rows, pitch), float("nan"), dtype=dtype)


def pack(img, pitch, offset, spare=0):
    """[M][C] -> [M + spare][pitch] with the image at channel offset, a sentinel everywhere else"""
    M, C = img.shape
    assert offset + C <= pitch
    buf = sentinel_buffer(M + spare, pitch, img.dtype)
    buf[:M, offset:offset + C] = img
    return buf


def unpack(buf, M, C, offset):
    return buf[:M, offset:offset + C]


def is_sentinel(t):
    t = t.detach().cpu()
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16) == torch.tensor(BF16_SENTINEL, dtype=torch.int16)
    return torch.isnan(t)


def outside_unchanged(buf, M, C, offset):
    """every element outside rows [0, M) x channels [offset, offset + C) still holds the sentinel"""
    s = is_sentinel(buf)
    inside = torch.zeros_like(s)
    inside[:M, offset:offset + C] = True
    return bool(s[~inside].all())


# ------------------------------------------------------------------ BatchNorm passes
def bn_vec(c, gen):
    """scale (either sign), beta, mean, invstd [4c], fp32"""
    sign = torch.where(torch.rand(c, generator=gen) < 0.25, -1.0, 1.0)
    return torch.cat([(torch.rand(c, generator=gen) + 0.5) * sign, torch.randn(c, generator=gen) * 0.3,
                      torch.randn(c, generator=gen) * 0.2, torch.rand(c, generator=gen) + 0.5])


def bnb_vec(c, bn, gen):
    """gi, m1, m2 drawn; mean, invstd those of bn [5c], fp32"""
    C = c
    return torch.cat([(torch.rand(c, generator=gen) + 0.5), torch.randn(c, generator=gen) * 0.3,
                      torch.randn(c, generator=gen) * 0.3, bn[2 * C:3 * C], bn[3 * C:4 * C]])


def pre_ref(z, bn):
    sc, be, mu = _d(bn).view(4, -1)[:3]
    return (_d(z) - mu) * sc + be


def decisive_z(m, bn, gen, dtype=torch.float32, margin=1e-3):
    """z [m][C] of dtype whose pre-activations (z - mean) * scale + beta all lie at least margin from zero: entries
    that are closer are redrawn farther out (on the dtype's grid, and re-checked after the rounding), so a kernel's
    few-ulp pre-activation has float64's sign and the ReLU mask can be demanded exactly. Nothing is excluded: the
    share of entries left out of a comparison is 0, asserted here."""
    C = bn.numel() // 4
    z = (torch.randn((m, C), generator=gen) * 2).to(dtype)
    for k in range(200):
        bad = pre_ref(z, bn).abs() < margin
        if not bad.any():
            break
        z[bad] = (torch.randn((m, C), generator=gen) * (2 + k))[bad].to(dtype)
    excluded = int((pre_ref(z, bn).abs() < margin).sum())
    assert excluded == 0, excluded
    return z


def bn_apply_ref(z, bn):
    """(relu((z - mean) * scale + beta), |z - mean| |scale| + |beta|) in float64 on the stored fp32 parameters"""
    sc, be, mu = _d(bn).view(4, -1)[:3]
    zc = _d(z) - mu
    return torch.relu(zc * sc + be), zc.abs() * sc.abs() + be.abs()


def bnbwd_terms(dh, z, bn):
    """(dm, dm * xhat) [M][C]: dm = dh * [pre > 0], xhat = (z - mean) * invstd"""
    sc, be, mu, inv = _d(bn).view(4, -1)
    dm = _d(dh) * (pre_ref(z, bn) > 0)
    return dm, dm * ((_d(z) - mu) * inv)


def bnbwd_finalize_ref(s1, s2, n, gamma, bn):
    """float64 finalize: bnb = gi, m1, m2, mean, invstd [5][C]; dgamma = sum dm xhat, dbeta = sum dm"""
    _, _, mu, inv = _d(bn).view(4, -1)
    return torch.stack([_d(gamma) * inv, s1 / n, s2 / n, mu, inv]), s2, s1


def bnbwd_apply_ref(dh, z, bn, bnb):
    """(dz, |gi| (|dm| + |m1| + |xhat m2|)) with dz = gi * (dm - m1 - xhat * m2), xhat from bnb's mean, invstd"""
    gi, m1, m2, mb, ib = _d(bnb).view(5, -1)
    dm = _d(dh) * (pre_ref(z, bn) > 0)
    xh = (_d(z) - mb) * ib
    return gi * (dm - m1 - xh * m2), gi.abs() * (dm.abs() + m1.abs() + (xh * m2).abs())


def tile_sums(v, tile):
    """column sums of v [n][C] per tile rows in float64: (sums [tiles][C], sums of |.|)"""
    v = _d(v)
    n, C = v.shape
    t = max((n + tile - 1) // tile, 1)
    p = torch.zeros((t * tile, C), dtype=torch.float64)
    p[:n] = v
    p = p.view(t, tile, C)
    return p.sum(1), p.abs().sum(1)


def wgrad_geometry(fmap, img):
    """(R, S, O) of a weight-gradient case; S2 reads an odd-sized source when the row count is odd"""
    B, H, W = img
    if fmap == S2:
        odd = npix(img) % 2
        return img, (B, 2 * H - odd, 2 * W - odd), img
    return geometry(fmap, img)


# weight-prep descriptors (kind, ci, co, taps, flip, co_src): Conv2d 3x3 plain and flipped, ConvTranspose2d k2 and
# k1, and Conv2d with fewer source rows than outputs (the padded rows must be zero); sizes off the 32 x 32 tile
WPREP_DESCS = [(0, 16, 64, 9, 0, 0), (0, 16, 64, 9, 1, 0), (0, 40, 24, 9, 1, 0), (0, 33, 65, 9, 0, 0),
               (1, 64, 16, 4, 0, 0), (1, 24, 40, 4, 0, 0), (1, 16, 64, 1, 0, 0), (1, 70, 34, 1, 0, 0),
               (0, 16, 64, 9, 0, 50), (0, 24, 128, 1, 0, 70), (0, 16, 32, 9, 1, 1), (0, 64, 64, 9, 0, 63)]
WPREP_HALVES = [(0, 16, 64, 9, 1, 0), (1, 24, 40, 4, 0, 0), (0, 16, 64, 9, 0, 50), (1, 16, 64, 1, 0, 0)]


def wprep_source_shape(kind, ci, co, taps, co_src):
    return (co_src or co, ci, taps) if kind == 0 else (ci, co, taps)


def wprep_ref(W, kind, co, flip):
    """(fwd [T][co][ci], dgrad [T][ci][co]) of the torch weight W ([co_src][ci][T] or [ci][co][T]): a permutation,
    rows past co_src zero, the data-gradient taps reversed when flip"""
    if kind == 0:
        Wp = torch.zeros((co, W.shape[1], W.shape[2]), dtype=W.dtype)
        Wp[:W.shape[0]] = W
        fwd, dgrad = Wp.permute(2, 0, 1), Wp.permute(2, 1, 0)
    else:
        fwd, dgrad = W.permute(2, 1, 0), W.permute(2, 0, 1)
    return fwd.contiguous(), (dgrad.flip(0) if flip else dgrad).contiguous()


def bf16_grid(*shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16)


def bf16_ties(n, gen):
    """fp32 values exactly halfway between two neighbouring bf16 values, either sign, even and odd lower neighbours"""
    base = (torch.randn(n, generator=gen)).to(torch.bfloat16).float()
    bits = base.view(torch.int32) | 0x8000          # the first dropped bit set, the rest zero: a tie
    return bits.view(torch.float32).clone()
