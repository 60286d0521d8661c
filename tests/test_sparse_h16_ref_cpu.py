"""The 16-bit reference helpers of tests/_sparse_cases.py (what tests/test_gpu_sparse_h16_kernels.py holds the HIP
kernels to) pinned against the existing conv_ref / dgrad_ref / wgrad_ref, plain loops and plain torch float64."""
import pytest
import torch

from tests import _sparse_cases as sc


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _identity_bnb(c):
    """gi 1, m1 0, m2 0, mean 0, invstd 1: bnbwd_ref returns dy itself with magnitude |dy|"""
    return torch.cat([torch.ones(c), torch.zeros(c), torch.zeros(c), torch.zeros(c), torch.ones(c)])


def _close(got, ref, S):
    assert ((got - ref).abs() <= 1e-13 * S).all()


@pytest.mark.parametrize("fmt", [0, 1])
def test_h16_grid_helpers(fmt):
    g = _gen(fmt)
    dt = sc.H16[fmt]
    assert [sc.r8(c) for c in (1, 8, 9, 20)] == [8, 8, 16, 24]
    assert [sc.r16(c) for c in (1, 16, 17, 120)] == [16, 16, 32, 128]
    assert [sc.r32(c) for c in (1, 32, 33, 100)] == [32, 32, 64, 128]
    h = sc.h16_rows(37, 20, g, fmt, scale=2.0)
    assert h.dtype == dt and h.shape == (37, 24)
    assert (h[:, 20:] == 0).all() and (h[:, :20] != 0).all()
    assert 1.5 < float(h[:, :20].float().std()) < 2.5
    W = sc.h16_weights(3, 5, 7, g, fmt)
    assert W.dtype == torch.float32 and W.shape == (3, 5, 7)
    assert torch.equal(W.to(dt).float(), W)                       # on the grid: rounding changes nothing


def test_saturating_rounding():
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([1e6, -7e4, 65504.0, 65519.0, 65520.0, -65520.0, 1.0, inf, -inf, nan, 0.1])
    s = sc.sat_f16(x)
    assert torch.equal(s[:9], torch.tensor([65504.0, -65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 1.0, inf, -inf]))
    assert torch.isnan(s[9]) and s[10] == x[10]
    h = sc.to_h16(x, 1)
    assert h.dtype == torch.float16
    assert torch.equal(h[:9].float(), s[:9]) and torch.isnan(h[9]) and h[10] == torch.tensor(0.1).half()
    b = sc.to_h16(x, 0)
    assert b.dtype == torch.bfloat16
    assert torch.equal(b[:9], x[:9].to(torch.bfloat16)) and float(b[0]) > 9e5     # bf16: torch's rounding, no clamp


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("dgrad", [0, 1])
def test_weight_tiles_ref_is_the_stated_layout(dgrad, fmt):
    K, ci, co = 3, 20, 40
    W = torch.randn((K, ci, co), generator=_gen(7)) * 0.1
    W[1, 2, 3] = 1e6
    t = sc.weight_tiles_ref(W, dgrad, fmt)
    n_, c_ = (ci, co) if dgrad else (co, ci)
    assert t.dtype == sc.H16[fmt] and t.shape == (K, sc.r16(n_), sc.r32(c_))
    for k in range(K):
        for n in range(t.shape[1]):
            for c in range(t.shape[2]):
                if n < n_ and c < c_:
                    w = W[k, n, c] if dgrad else W[k, c, n]
                    want = w.clamp(-65504.0, 65504.0).to(torch.float16) if fmt else w.to(torch.bfloat16)
                    assert t[k, n, c] == want
                else:
                    assert t[k, n, c] == 0


@pytest.mark.parametrize("n_out,K", [(1, 3), (70, 27), (200, 27)])
def test_gather_gemm_ref_against_conv_ref_and_dgrad_ref(n_out, K):
    g = _gen(n_out + K)
    kg, ng, n_src = 20, 24, 50
    a = sc.h16_rows(n_src, kg, g, 0)                              # 24 columns: the reference reads the first 20
    W = sc.h16_weights(K, kg, ng, g, 0)
    mp = sc.random_map(n_out, n_src, K, seed=n_out)
    out, S = sc.gather_gemm_ref(a, mp, 0, W)
    ref, Sr, _ = sc.conv_ref(a[:, :kg].float(), mp, W)
    _close(out, ref, Sr)
    _close(S, Sr, Sr)
    assert (S[0] > 0).all()
    # the data gradient's form: rows of width co through the transposed W [K, ci, co], both orders of the offsets
    dy = sc.h16_rows(n_src, ng, g, 0)
    zz = torch.randn((n_src, ng), generator=g)
    for rev in (0, 1):
        out, S = sc.gather_gemm_ref(dy, mp, rev, W.transpose(1, 2))
        ref, Sr, _ = sc.dgrad_ref(dy.float(), zz, _identity_bnb(ng), mp, rev, W)
        _close(out, ref, Sr)
        _close(S, Sr, Sr)
    a0 = sc.gather_gemm_ref(dy, mp, 0, W.transpose(1, 2))[0]
    assert not torch.equal(a0, out)                               # the map is not symmetric: rev matters


def test_gather_gemm_ref_rev_by_plain_loops():
    g = _gen(5)
    K, kg, ng = 3, 2, 3
    a = torch.randn((4, kg), generator=g)
    B = torch.randn((K, kg, ng), generator=g)
    mp = torch.tensor([[0, -1, 3], [2, 2, -1], [-1, -1, -1]])
    for rev in (0, 1):
        want = torch.zeros((3, ng), dtype=torch.float64)
        for r in range(3):
            for k in range(K):
                src = int(mp[r, K - 1 - k if rev else k])
                if src >= 0:
                    for c in range(kg):
                        for n in range(ng):
                            want[r, n] += float(a[src, c]) * float(B[k, c, n])
        out, S = sc.gather_gemm_ref(a, mp, rev, B)
        assert torch.allclose(out, want, rtol=0, atol=1e-14)
        assert (out[2] == 0).all() and (S[2] == 0).all() and (S >= out.abs() - 1e-14).all()


@pytest.mark.parametrize("n_out,K", [(1, 3), (130, 27)])
def test_gather_wgrad_ref_against_wgrad_ref(n_out, K):
    g = _gen(11 * n_out + K)
    ci, co, n_src = 16, 32, 40
    h = sc.h16_rows(n_src, ci, g, 0)
    dz = sc.h16_rows(n_out, co, g, 0)
    nbr = sc.random_map(n_out, n_src, K, seed=K)
    dW, S, nk = sc.gather_wgrad_ref(h, nbr, dz)
    ref, Sr, _ = sc.wgrad_ref(h.float(), None, nbr, dz.float(), torch.randn((n_out, co), generator=g),
                              _identity_bnb(co))
    _close(dW, ref, Sr)
    _close(S, Sr, Sr)
    assert torch.equal(nk, (nbr >= 0).sum(0)) and nk[1] == 0 and (dW[1] == 0).all()
    if n_out > 63:
        assert nk[K - 1] == 1


@pytest.mark.parametrize("with_res", [False, True])
def test_infer_ref_is_plain_torch(with_res):
    g = _gen(3)
    acc = torch.randn((9, 5), generator=g, dtype=torch.float64)
    fold = torch.randn(10, generator=g)
    res = torch.randn((9, 5), generator=g) if with_res else None
    y, M = sc.infer_ref(acc, fold, res)
    sc_, sh = fold.double()[:5], fold.double()[5:]
    pre = acc * sc_ + sh + (res.double() if with_res else 0.0)
    assert torch.equal(y, torch.nn.functional.relu(pre))
    assert torch.equal(M, (acc * sc_).abs() + sh.abs() + (res.double().abs() if with_res else 0.0))
    assert (y == 0).any() and (y > 0).any() and (M >= pre.abs() - 1e-15).all()
