"""The fp32 sparse-conv kernels in isolation through the C ABI: rpc_spconv_forward / _dgrad / _wgrad (the MFMA
k_gemm and k_wgrad, and the narrow k_l0_fwd / k_l0_dgrad / k_wgrad_narrow of the 4- and 5-channel input layer),
rpc_sparse_to_dense / rpc_dense_to_sparse_grad and rpc_sparse_res_forward(_h16), element by element against the
float64 references of tests/_sparse_cases.py.

Bounds. u = 2^-24. An fp32 sum of n products in any order lies within n * u * S of the exact one, S the sum of the
magnitudes of its terms; the tests allow (n + 8) * u * S, the 8 for the roundings of the operand formed on load
(BatchNorm backward: 6 roundings relative to |gi| * (|dy| + |m1| + |xhat| * |m2|), which is what S is taken
over). The ReLU decisions behind every mask are drawn at least 1e-3 from 0, far beyond the two roundings of
fma(x - mean, scale, beta), so the masks are demanded exactly.

One step is added to the weight gradient's bound. Its forward operand A = relu(fma(x - mean, scale, beta)) rounds
twice relative to M = |x - mean| * |scale| + |beta|, not relative to its own, cancelled, value: an operand 100
times smaller than M carries 100 times the relative error, and with a single term in the sum (n_out = 1) no
multiple of u * |A| * |dz| covers it. On the MI355X the bound without this step is missed for n_out = 1 with in_bn
on four pairs, by up to 2.7 times, and by nothing else. The step is added as it is: 2 * u * T, T = sum M |dz|.
The forward forms the same operand; it has K * CI >= 12 terms' worth of allowance and is held to the bound as
stated, without this step."""
import zlib

import numpy as np
import pytest
import torch

from robustpointclouds_amd import _ffi
from tests import _sparse_cases as sc
from tests._sparse_hip import hip_strided, hip_subm, index_grid

pytestmark = pytest.mark.gpu

U = sc.U
PAIRS = [(4, 16), (5, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (64, 16), (128, 128)]
N_SRC = 300
ROWS = [1, 63, 64, 65, 577]               # 577: 10 tiles, more than the 8 XCDs the block remap spreads over
WG_ROWS = [1, 257, 513, 2049, 4100]       # across the narrow kernel's 256-row and the general one's 2048-row chunks
KS = [27, 3]
SPARE = 70                                # rows allocated beyond n_out, NaN-filled: nothing may write them
RPC_ERR_WORKSPACE, RPC_ERR_UNSUPPORTED = 2, 3


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _within(got, ref, tol, what):
    err = (got - ref).abs()
    bad = ~(err <= tol)                    # a NaN counts as bad
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), float((err / tol.clamp_min(1e-300))[bad].max()))


def _tiles(n):
    return (n + sc.TILE - 1) // sc.TILE


def _check_part(part, v, w, what):
    """partial rows [tiles, 2C] = per-tile column sums of the stored rows v and of v * w, in float64 within 72 u of
    their magnitudes (64 additions, the product, and the two roundings of an xhat formed in fp32)"""
    C = v.shape[1]
    p = part.cpu().double()
    s1, a1 = sc.tile_sums(v)
    s2, a2 = sc.tile_sums(v * w)
    _within(p[:, :C], s1, 72 * U * a1, what + " part[0]")
    _within(p[:, C:], s2, 72 * U * a2, what + " part[1]")


# ------------------------------------------------------------------ forward
def _forward(lib, xd, bnd, ci, nd, K, n_out, Wd, co, with_part):
    dev = xd.device
    z = _nan((n_out + SPARE, co), dev)
    part = _nan((_tiles(n_out), 2 * co), dev) if with_part else None
    _ffi.check(lib.rpc_spconv_forward(_ffi.ptr(xd), _ffi.ptr(bnd), ci, _ffi.ptr(nd), K, n_out, _ffi.ptr(Wd), co,
                                      _ffi.ptr(z), _ffi.ptr(part), _ffi.stream_of(z)), "rpc_spconv_forward")
    torch.cuda.synchronize()
    return z, part


@pytest.mark.parametrize("n_out", ROWS)
@pytest.mark.parametrize("ci,co", PAIRS)
def test_forward_matches_fp64(ci, co, n_out):
    lib = _ffi.load()
    dev = torch.device("cuda")
    for K in KS:
        g = _gen("fwd", ci, co, n_out, K)
        x = torch.randn((N_SRC, ci), generator=g) * 2
        W = torch.randn((K, ci, co), generator=g) * 0.1
        nbr = sc.random_map(n_out, N_SRC, K, seed=ci * 131 + co + n_out + K)
        xd, Wd, nd = x.to(dev), W.to(dev), nbr.to(dev)
        for bn in (None, sc.bn_vec(ci, g)):
            what = f"forward ({ci},{co}) n_out {n_out} K {K} bn {bn is not None}"
            ref, S, _ = sc.conv_ref(x, nbr, W, bn)
            bnd = None if bn is None else bn.to(dev)
            z, part = _forward(lib, xd, bnd, ci, nd, K, n_out, Wd, co, True)
            got = z[:n_out].cpu().double()
            _within(got, ref, (K * ci + 8) * U * S, what)
            assert torch.isnan(z[n_out:]).all(), what
            if n_out > 127:
                assert (z[64:128] == 0).all(), what             # a tile without any neighbour
            assert bn is not None or (ref[0] != 0).all()        # row 0 always has a neighbour
            _check_part(part, got, got, what)
            z2, _ = _forward(lib, xd, bnd, ci, nd, K, n_out, Wd, co, False)
            assert torch.equal(z2[:n_out], z[:n_out]) and torch.isnan(z2[n_out:]).all(), what


# ------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("ci,co", PAIRS)
def test_dgrad_matches_fp64(ci, co, n):
    """din [n, ci] from dz rows [N_SRC, co] through map [n, K]: the transposed pairs of the forward list"""
    lib = _ffi.load()
    dev = torch.device("cuda")
    for K in KS:
        g = _gen("dgrad", ci, co, n, K)
        dy = torch.randn((N_SRC, co), generator=g)
        zz = torch.randn((N_SRC, co), generator=g) * 2
        bnb = sc.bnb_vec(co, g)
        W = torch.randn((K, ci, co), generator=g) * 0.1
        mp = sc.random_map(n, N_SRC, K, seed=ci * 137 + co + n + K)
        prev_bn = sc.bn_vec(ci, g)
        prev_z = sc.decisive_z(n, prev_bn, g)
        dyd, zd, bd, Wd, md = dy.to(dev), zz.to(dev), bnb.to(dev), W.to(dev), mp.to(dev)
        pzd, pbd = prev_z.to(dev), prev_bn.to(dev)
        st = _ffi.stream_of(dyd)
        for rev in (0, 1):
            for masked in ((False, True) if ci >= 16 else (False,)):
                what = f"dgrad ({ci},{co}) n {n} K {K} rev {rev} masked {masked}"
                ref, S, xh = sc.dgrad_ref(dy, zz, bnb, mp, rev, W, prev_z if masked else None,
                                          prev_bn if masked else None)
                din = _nan((n + SPARE, ci), dev)
                part = _nan((_tiles(n), 2 * ci), dev) if masked else None
                _ffi.check(lib.rpc_spconv_dgrad(_ffi.ptr(dyd), _ffi.ptr(zd), _ffi.ptr(bd), co, _ffi.ptr(md), K, rev, n,
                                                _ffi.ptr(Wd), ci, _ffi.ptr(pzd) if masked else None,
                                                _ffi.ptr(pbd) if masked else None, _ffi.ptr(din), _ffi.ptr(part), st),
                           "rpc_spconv_dgrad")
                torch.cuda.synchronize()
                got = din[:n].cpu().double()
                _within(got, ref, (K * co + 8) * U * S, what)
                assert torch.isnan(din[n:]).all(), what
                if n > 127:
                    assert (din[64:128] == 0).all(), what
                if masked:
                    keep = sc.relu_mask_ref(prev_z, prev_bn)
                    assert (got[~keep] == 0).all() and (got[keep] != 0).any(), what     # the exact mask
                    _check_part(part, got, xh, what)


# ------------------------------------------------------------------ weight gradient
def _wgrad(lib, xd, bnd, ci, nd, K, n_out, dyd, zd, bd, co, ws, wsz):
    dW = _nan((K, ci, co), xd.device)
    _ffi.check(lib.rpc_spconv_wgrad(_ffi.ptr(xd), _ffi.ptr(bnd), ci, _ffi.ptr(nd), K, n_out, _ffi.ptr(dyd),
                                    _ffi.ptr(zd), _ffi.ptr(bd), co, _ffi.ptr(dW), _ffi.ptr(ws), wsz,
                                    _ffi.stream_of(dW)), "rpc_spconv_wgrad")
    torch.cuda.synchronize()
    return dW


@pytest.mark.parametrize("n_out", WG_ROWS)
@pytest.mark.parametrize("ci,co", PAIRS)
def test_wgrad_matches_fp64(ci, co, n_out):
    lib = _ffi.load()
    dev = torch.device("cuda")
    for K in KS:
        g = _gen("wgrad", ci, co, n_out, K)
        x = torch.randn((N_SRC, ci), generator=g) * 2
        dy = torch.randn((n_out, co), generator=g)
        zz = torch.randn((n_out, co), generator=g) * 2
        bnb = sc.bnb_vec(co, g)
        nbr = sc.random_map(n_out, N_SRC, K, seed=ci * 139 + co + n_out + K)
        xd, dyd, zd, bd, nd = x.to(dev), dy.to(dev), zz.to(dev), bnb.to(dev), nbr.to(dev)
        wsz = lib.rpc_spconv_wgrad_workspace_size(n_out, K, ci, co)
        ws = _ffi.workspace(wsz, dev)
        for bn in (None, sc.bn_vec(ci, g)):
            what = f"wgrad ({ci},{co}) n_out {n_out} K {K} bn {bn is not None}"
            ref, S, T = sc.wgrad_ref(x, bn, nbr, dy, zz, bnb)
            bnd = None if bn is None else bn.to(dev)
            dW = _wgrad(lib, xd, bnd, ci, nd, K, n_out, dyd, zd, bd, co, ws, wsz)
            # + 2 u T: the on-load transform's two roundings, relative to M (module docstring)
            _within(dW.cpu().double(), ref, (n_out + 8) * U * S + 2 * U * T, what)
            assert (dW[1] == 0).all(), what                      # the offset nobody uses
            if n_out > 63 and bn is None:
                assert (ref[K - 1] != 0).all()                    # the offset only row 63 uses: one term each
            assert torch.equal(dW, _wgrad(lib, xd, bnd, ci, nd, K, n_out, dyd, zd, bd, co, ws, wsz)), what


def test_conv_argument_handling():
    lib = _ffi.load()
    dev = torch.device("cuda")
    n_out, K, ci, co = 100, 27, 16, 16
    g = _gen("args")
    x, dy, zz = (torch.randn((n_out, 24), generator=g).to(dev) for _ in range(3))
    bnb = sc.bnb_vec(24, g).to(dev)
    nbr = sc.random_map(n_out, n_out, K, seed=3).to(dev)
    W = torch.randn((K, 24, 24), generator=g).to(dev)
    st = _ffi.stream_of(x)
    wsz = lib.rpc_spconv_wgrad_workspace_size(n_out, K, ci, co)
    ws = _ffi.workspace(max(wsz, lib.rpc_spconv_wgrad_workspace_size(n_out, K, 24, 16)), dev)
    dW = torch.full((K, 24, 24), 1.0, device=dev)
    call = lambda c_i, c_o, n, nbytes: lib.rpc_spconv_wgrad(_ffi.ptr(x), None, c_i, _ffi.ptr(nbr), K, n, _ffi.ptr(dy),
                                                            _ffi.ptr(zz), _ffi.ptr(bnb), c_o, _ffi.ptr(dW),
                                                            _ffi.ptr(ws), nbytes, st)
    assert call(ci, co, n_out, wsz - 4) == RPC_ERR_WORKSPACE
    assert call(24, 16, n_out, ws.numel()) == RPC_ERR_UNSUPPORTED
    z = torch.full((n_out, 24), 1.0, device=dev)
    assert lib.rpc_spconv_forward(_ffi.ptr(x), None, 24, _ffi.ptr(nbr), K, n_out, _ffi.ptr(W), 16, _ffi.ptr(z), None,
                                  st) == RPC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (dW == 1).all() and (z == 1).all()                    # the refusals wrote nothing
    _ffi.check(call(ci, co, 0, wsz), "rpc_spconv_wgrad(empty)")
    torch.cuda.synchronize()
    flat = dW.flatten()
    assert (flat[:K * ci * co] == 0).all() and (flat[K * ci * co:] == 1).all()


# ------------------------------------------------------------------ rulebook + forward against a dense operation
def test_rulebook_and_forward_chain_matches_dense_conv3d():
    """HIP SubM rulebook + forward (16 -> 32), then HIP strided rulebook + forward (32 -> 64) on the first one's
    stored rows, each against float64 conv3d of the densified input read back at the output sites."""
    lib = _ffi.load()
    dev = torch.device("cuda")
    shape, geom = sc.GRIDS[0], sc.GEOMS[0]
    coors = sc.corner_case_coors(shape, 130, seed=1)
    g = _gen("chain")
    x = torch.randn((130, 16), generator=g)
    W1 = torch.randn((27, 16, 32), generator=g) * 0.1
    W2 = torch.randn((27, 32, 64), generator=g) * 0.1
    nbr = hip_subm(coors, shape, index_grid(shape, dev))
    z1, _ = _forward(lib, x.to(dev), None, 16, nbr, 27, 130, W1.to(dev), 32, False)
    z1 = z1[:130]
    dense, S = sc.dense_conv_ref(x, coors, shape, W1, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    _within(z1.cpu().double(), sc.read_sites(dense, coors), (27 * 16 + 8) * U * sc.read_sites(S, coors), "subm chain")
    n_out, coors_out, nbr_out, _ = hip_strided(coors, shape, geom, index_grid(sc.out_shape(shape, *geom), dev))
    assert n_out == len(sc.strided_rulebook(coors, shape, *geom)[0])
    z2, _ = _forward(lib, z1.contiguous(), None, 32, nbr_out, 27, n_out, W2.to(dev), 64, False)
    co = coors_out.cpu().numpy()
    dense2, S2 = sc.dense_conv_ref(z1.cpu(), coors, shape, W2, *geom)
    _within(z2[:n_out].cpu().double(), sc.read_sites(dense2, co), (27 * 32 + 8) * U * sc.read_sites(S2, co),
            "strided chain")


# ------------------------------------------------------------------ dense scatter / gather
DSHAPE = (2, 2, 5, 7)


def _dense_case(C, flags, n):
    B, D, H, W = DSHAPE
    g = _gen("dense", C, flags, n)
    cells = B * D * H * W
    pick = [cells - 1] if n == 1 else torch.randperm(cells, generator=g)[:n].tolist()
    coors = np.asarray([np.unravel_index(i, DSHAPE) for i in pick], np.int32)
    bn = sc.bn_vec(C, g)
    z = sc.decisive_z(n, bn, g)
    return g, coors, bn, z


def _image(rows, coors, C, nhwc):
    """rows [n, C] scattered into zeros as [B, C*D, H, W] (channel c * D + z), or its NHWC form"""
    B, D, H, W = DSHAPE
    c = torch.from_numpy(coors).long()
    img = torch.zeros((B, C, D, H, W), dtype=rows.dtype)
    img[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = rows
    img = img.view(B, C * D, H, W)
    return img.permute(0, 2, 3, 1).contiguous() if nhwc else img


@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [6, 16, 128])
def test_sparse_to_dense_and_back(C, flags, n):
    lib = _ffi.load()
    dev = torch.device("cuda")
    B, D, H, W = DSHAPE
    nhwc, bf16 = bool(flags & 1), bool(flags & 2)
    g, coors, bn, z = _dense_case(C, flags, n)
    zd, bd, cd = z.to(dev), bn.to(dev), torch.from_numpy(coors).to(dev)
    dshape = (B, H, W, C * D) if nhwc else (B, C * D, H, W)
    dense = torch.zeros(dshape, dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    st = _ffi.stream_of(dense)
    shp = _ffi.int_arr(DSHAPE)
    _ffi.check(lib.rpc_sparse_to_dense(_ffi.ptr(zd), _ffi.ptr(bd), _ffi.ptr(cd), n, C, shp, flags, _ffi.ptr(dense), st),
               "rpc_sparse_to_dense")
    torch.cuda.synchronize()
    A, M = sc.act_ref(z, bn)
    want = _image(A, coors, C, nhwc)
    # fp32: x - mean, the fused multiply-add (2 roundings relative to M; 4 allowed). bf16: one bf16 ulp (<= 2^-7
    # |value|) of the float64 value. Unoccupied cells: tolerance 0, exactly 0.
    tol = _image(A * 2.0 ** -7 if bf16 else 4 * U * M, coors, C, nhwc)
    _within(dense.cpu().double(), want, tol, f"to_dense C {C} flags {flags} n {n}")
    assert int((dense != 0).sum()) == int((A > 0).sum())
    # backward: the dense gradient gathered under the exact mask, and its BatchNorm-backward partial rows
    gd = torch.randn(dshape, generator=g)
    gd = gd.to(torch.bfloat16) if bf16 else gd
    gdd = gd.to(dev)
    dy = _nan((n + SPARE, C), dev)
    part = _nan((_tiles(n), 2 * C), dev)
    _ffi.check(lib.rpc_dense_to_sparse_grad(_ffi.ptr(gdd), _ffi.ptr(zd), _ffi.ptr(bd), _ffi.ptr(cd), n, C, shp, flags,
                                            _ffi.ptr(dy), _ffi.ptr(part), st), "rpc_dense_to_sparse_grad")
    torch.cuda.synchronize()
    c = torch.from_numpy(coors).long()
    gf = gd.float()
    if nhwc:
        rows = gf.view(B, H, W, C, D)[c[:, 0], c[:, 2], c[:, 3], :, c[:, 1]]
    else:
        rows = gf.view(B, C, D, H, W)[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]
    keep = sc.relu_mask_ref(z, bn)
    assert torch.equal(dy[:n].cpu(), rows * keep.float())
    assert torch.isnan(dy[n:]).all()
    sc_, be_, mu_, is_ = bn.double().view(4, C)
    _check_part(part, dy[:n].cpu().double(), (z.double() - mu_) * is_, f"from_dense C {C} flags {flags} n {n}")


# ------------------------------------------------------------------ residual rows
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("n", [1, 65, 300])
@pytest.mark.parametrize("c", [16, 20, 128])
def test_sparse_res_forward_rows(c, n, with_res):
    """out = relu(bn(z) + res): fp32 rows within 4 u of the term magnitudes (x - mean, the fused multiply-add, the
    residual add: 3 roundings), 16-bit rows within one ulp of their format of the float64 value, padding columns 0,
    and a row of 1e6 saturating to 65504 in fp16."""
    lib = _ffi.load()
    dev = torch.device("cuda")
    g = _gen("res", c, n, with_res)
    cp = (c + 7) // 8 * 8
    bn = sc.bn_vec(c, g)
    z = torch.randn((n, c), generator=g) * 2
    res = torch.randn((n, c), generator=g) if with_res else None
    if with_res:
        res[n - 1] = 1e6
    else:
        z[n - 1] = bn[2 * c:3 * c] + 1e6 / bn[:c]            # (z - mean) * scale = 1e6 whatever the sign of scale
    zd, bd = z.to(dev), bn.to(dev)
    rd = res.to(dev) if with_res else None
    st = _ffi.stream_of(zd)
    sc_, be_, mu_ = bn.double().view(4, c)[:3]
    pre = (z.double() - mu_) * sc_ + be_ + (res.double() if with_res else 0.0)
    want = torch.relu(pre)
    M = (z.double() - mu_).abs() * sc_.abs() + be_.abs() + (res.double().abs() if with_res else 0.0)
    assert (want[n - 1] > 9e5).all()
    outs = []
    for fmt in (0, 1):
        what = f"res_forward c {c} n {n} res {with_res} fmt {fmt}"
        out = _nan((n + SPARE, c), dev)
        h = torch.full((n, cp), 7.0, dtype=torch.float16 if fmt else torch.bfloat16, device=dev)
        hb = torch.full((n, cp), 7.0, dtype=torch.bfloat16, device=dev)
        if fmt:
            _ffi.check(lib.rpc_sparse_res_forward_h16(_ffi.ptr(zd), _ffi.ptr(bd), _ffi.ptr(rd), n, c, _ffi.ptr(out),
                                                      _ffi.ptr(h), 1, _ffi.ptr(hb), st), "rpc_sparse_res_forward_h16")
        else:
            _ffi.check(lib.rpc_sparse_res_forward(_ffi.ptr(zd), _ffi.ptr(bd), _ffi.ptr(rd), n, c, _ffi.ptr(out),
                                                  _ffi.ptr(h), st), "rpc_sparse_res_forward")
        torch.cuda.synchronize()
        _within(out[:n].cpu().double(), want, 4 * U * M, what)
        assert torch.isnan(out[n:]).all(), what
        outs.append(out[:n].clone())
        # the 16-bit rows: the kernel's own fp32 row rounded to nearest even (fp16: saturated first), bit for bit,
        # and within one ulp of the format of the float64 value (fp16: 2^-10 |value|, 2^-24 below the normal range)
        o32 = out[:n].cpu()
        if fmt:
            sat = want.clamp(max=65504.0)
            assert torch.equal(h[:, :c].cpu(), o32.clamp(max=65504.0).to(torch.float16)), what
            _within(h[:, :c].cpu().double(), sat, sat * 2.0 ** -10 + 2.0 ** -24, what + " fp16 rows")
            assert (h[n - 1, :c] == 65504.0).all(), what
        for b in ([hb] if fmt else [h]):
            assert torch.equal(b[:, :c].cpu(), o32.to(torch.bfloat16)), what
            _within(b[:, :c].cpu().double(), want, want * 2.0 ** -7, what + " bf16 rows")
            assert (b[:, c:] == 0).all(), what
        assert (h[:, c:] == 0).all(), what
    assert torch.equal(outs[0], outs[1])
