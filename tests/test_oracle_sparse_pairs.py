"""The oracle's rulebooks (oracle.sparse_encoder.subm_pairs / spconv_pairs) against brute force over a dict from
coordinate to row, and the float64 sparse-conv reference of tests/_sparse_cases.py against torch's dense conv3d:
the offset convention k = (kz * kh + ky) * kw + kx and the W[k][CI][CO] layout pinned to an independent operation.
Runs without a GPU."""
import numpy as np
import pytest
import torch

from oracle.sparse_encoder import spconv_pairs, subm_pairs
from tests import _sparse_cases as sc

N = 130


def _oracle_set(pairs, coors_in, coors_out):
    s = set()
    for k, (ri, ro) in enumerate(pairs):
        for a, b in zip(coors_in[ri].tolist(), coors_out[ro].tolist()):
            s.add((k, tuple(a), tuple(b)))
    assert len(s) == sum(len(ri) for ri, _ in pairs)
    return s


@pytest.mark.parametrize("shape", sc.GRIDS)
def test_subm_pairs_match_brute_force(shape):
    coors = sc.corner_case_coors(shape, N, seed=1)
    nbr = sc.subm_rulebook(coors)
    got = _oracle_set(subm_pairs(coors.astype(np.int64), shape), coors, coors)
    want = sc.pair_set(nbr, coors, coors)
    assert got == want and len(want) > N
    # the properties the voxel set promises: the centre is the row itself, one voxel has no neighbour, and the
    # two cells adjacent in the linear grid across the frame seam are not neighbours
    assert (nbr[:, 13] == np.arange(N)).all()
    assert ((nbr >= 0).sum(1) == 1).any()
    row = {tuple(c): r for r, c in enumerate(coors.tolist())}
    B, D, H, W = shape
    last0, first1 = row[(0, D - 1, H - 1, W - 1)], row[(1, 0, 0, 0)]
    assert first1 not in nbr[last0] and last0 not in nbr[first1]


@pytest.mark.parametrize("shape", sc.GRIDS)
def test_brute_force_subm_rulebook_is_symmetric(shape):
    """the brute-force map checks itself: N centres, and i is j's neighbour through k iff j is i's through 26 - k"""
    nbr = sc.subm_rulebook(sc.corner_case_coors(shape, N, seed=1))
    r, k = np.nonzero(nbr >= 0)
    assert (nbr[nbr[r, k], 26 - k] == r).all()
    cnt = int((nbr >= 0).sum())
    assert cnt >= N and (cnt - N) % 2 == 0
    for k in range(27):     # offset k and its mirror pair the same voxels
        assert (nbr[:, k] >= 0).sum() == (nbr[:, 26 - k] >= 0).sum()


@pytest.mark.parametrize("geom", sc.GEOMS)
@pytest.mark.parametrize("shape", sc.GRIDS)
def test_spconv_pairs_match_brute_force(shape, geom):
    ksize, stride, pad = geom
    coors = sc.corner_case_coors(shape, N, seed=1)
    coors_out, nbr_out, nbr_in = sc.strided_rulebook(coors, shape, ksize, stride, pad)
    oshape = sc.out_shape(shape, ksize, stride, pad)
    oc, pairs = spconv_pairs(coors.astype(np.int64), oshape, ksize, stride, pad)
    assert {tuple(c) for c in oc.tolist()} == {tuple(c) for c in coors_out.tolist()}
    assert len(oc) == len(coors_out) > 0
    assert _oracle_set(pairs, coors, oc) == sc.pair_set(nbr_out, coors, coors_out)
    # the two brute-force maps are each other's inverse, and every output row is reached
    o, k = np.nonzero(nbr_out >= 0)
    assert (nbr_in[nbr_out[o, k], k] == o).all() and (nbr_in >= 0).sum() == len(o)
    assert (nbr_out >= 0).any(1).all()
    assert (coors_out[:, 1:] < np.asarray(oshape[1:])).all() and (coors_out >= 0).all()


def _rows(n, c, seed):
    return torch.randn((n, c), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("shape", sc.GRIDS)
def test_conv_ref_subm_equals_dense_conv3d(shape):
    ci, co = 5, 7
    coors = sc.corner_case_coors(shape, N, seed=2)
    x, W = _rows(N, ci, 3), _rows(27 * ci, co, 4).view(27, ci, co)
    z, S, _ = sc.conv_ref(x, sc.subm_rulebook(coors), W)
    dense, _ = sc.dense_conv_ref(x, coors, shape, W, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    want = sc.read_sites(dense, coors)
    assert S.min() > 0
    assert ((z - want).abs() <= 1e-12 * S).all()


@pytest.mark.parametrize("geom", sc.GEOMS)
@pytest.mark.parametrize("shape", sc.GRIDS)
def test_conv_ref_strided_equals_dense_conv3d(shape, geom):
    ksize, stride, pad = geom
    K = ksize[0] * ksize[1] * ksize[2]
    ci, co = 5, 7
    coors = sc.corner_case_coors(shape, N, seed=2)
    coors_out, nbr_out, _ = sc.strided_rulebook(coors, shape, ksize, stride, pad)
    x, W = _rows(N, ci, 5), _rows(K * ci, co, 6).view(K, ci, co)
    z, S, _ = sc.conv_ref(x, nbr_out, W)
    dense, _ = sc.dense_conv_ref(x, coors, shape, W, ksize, stride, pad)
    assert tuple(dense.shape) == (shape[0], co) + sc.out_shape(shape, ksize, stride, pad)[1:]
    assert ((z - sc.read_sites(dense, coors_out)).abs() <= 1e-12 * S).all()
    # every cell that is no output site is exactly 0 in the dense result
    site = torch.zeros(dense.shape[:1] + dense.shape[2:], dtype=torch.bool)
    c = torch.from_numpy(coors_out).long()
    site[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = True
    assert (dense.permute(0, 2, 3, 4, 1)[~site] == 0).all()


def test_conv_ref_applies_the_on_load_transform():
    """A = relu((x - mean) * scale + beta) on the gathered rows, against the same convolution of pre-transformed rows"""
    g = torch.Generator().manual_seed(7)
    bn = sc.bn_vec(5, g)
    x = _rows(40, 5, 8)
    nbr = sc.random_map(130, 40, 27, 9)
    W = _rows(27 * 5, 16, 10).view(27, 5, 16)
    A, M = sc.act_ref(x, bn)
    z0, S0, _ = sc.conv_ref(A, nbr, W)
    z1, S1, T1 = sc.conv_ref(x, nbr, W, bn)
    assert torch.equal(z0, z1) and torch.equal(S0, S1) and (T1 >= S1).all()
    assert (A >= 0).all() and (A == 0).any() and (M >= A).all()
    assert (z1[64:128] == 0).all() and (z1[128:] != 0).any() and (nbr[:, 1] == -1).all() and (nbr[:63, 26] == -1).all() and nbr[63, 26] >= 0


def test_gradient_refs_are_the_adjoints_of_conv_ref():
    """dgrad_ref and wgrad_ref against autograd of conv_ref's own formula: <dz, conv(x)> differentiated in x (through
    the inverse map, both column orders) and in W"""
    g = torch.Generator().manual_seed(11)
    n_in, n_out, K, ci, co = 30, 45, 27, 4, 6
    coors = sc.corner_case_coors(sc.GRIDS[0], n_in, seed=3)
    nbr = sc.subm_rulebook(coors)          # SubM: the map is its own inverse under k -> K-1-k
    x = _rows(n_in, ci, 12).requires_grad_(True)
    W = _rows(K * ci, co, 13).view(K, ci, co).clone().requires_grad_(True)
    z = torch.zeros((n_in, co), dtype=torch.float64)
    nb = torch.from_numpy(nbr).long()
    for k in range(K):
        ok = nb[:, k] >= 0
        z = z.index_add(0, torch.nonzero(ok)[:, 0], x[nb[ok, k]] @ W[k])
    dy, zz = _rows(n_in, co, 14), _rows(n_in, co, 15)
    bnb = sc.bnb_vec(co, g)
    dz, mag = sc.bnbwd_ref(dy, zz, bnb)
    assert (mag >= dz.abs() - 1e-15).all()
    (z * dz).sum().backward()
    din, S, _ = sc.dgrad_ref(dy, zz, bnb, nbr, True, W.detach())
    assert ((din - x.grad).abs() <= 1e-12 * S).all()
    dW, SW, _ = sc.wgrad_ref(x.detach(), None, nbr, dy, zz, bnb)
    assert ((dW - W.grad).abs() <= 1e-12 * SW).all()
    # a strided conv: the data gradient runs over nbr_in with the offsets in forward order (rev = 0)
    co_, nbr_out, nbr_in = sc.strided_rulebook(coors, sc.GRIDS[0], *sc.GEOMS[0])
    n_out = len(co_)
    x2 = _rows(n_in, ci, 16).requires_grad_(True)
    nb = torch.from_numpy(nbr_out).long()
    z2 = torch.zeros((n_out, co), dtype=torch.float64)
    for k in range(K):
        ok = nb[:, k] >= 0
        z2 = z2.index_add(0, torch.nonzero(ok)[:, 0], x2[nb[ok, k]] @ W.detach()[k])
    dy2, zz2 = _rows(n_out, co, 17), _rows(n_out, co, 18)
    dz2, _ = sc.bnbwd_ref(dy2, zz2, bnb)
    (z2 * dz2).sum().backward()
    din2, S2, _ = sc.dgrad_ref(dy2, zz2, bnb, nbr_in, False, W.detach())
    assert ((din2 - x2.grad).abs() <= 1e-12 * S2).all()


def test_tile_sums_and_decisive_rows():
    v = _rows(130, 3, 19)
    s, a = sc.tile_sums(v)
    assert s.shape == (3, 3)
    assert torch.allclose(s[1], v[64:128].sum(0), rtol=0, atol=1e-12) and torch.allclose(s[2], v[128:].sum(0), atol=1e-12)
    assert torch.allclose(a.sum(0), v.abs().sum(0), atol=1e-12)
    g = torch.Generator().manual_seed(20)
    bn = sc.bn_vec(16, g)
    z = sc.decisive_z(300, bn, g)
    s_, b_, m_ = bn.double().view(4, 16)[:3]
    assert (((z.double() - m_) * s_ + b_).abs() >= 1e-3).all()
    assert 0.2 < sc.relu_mask_ref(z, bn).double().mean() < 0.8
