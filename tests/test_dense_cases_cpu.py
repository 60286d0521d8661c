"""Pins the float64 references of tests/_dense_cases.py on the CPU: the BatchNorm-backward formulas against torch
autograd, the pitched-buffer helpers, the map references against an explicit gather loop over src_row as
csrc/dense_common.h writes it, and the ReLU-margin generator on every case of the lists."""
import pytest
import torch
import torch.nn.functional as F

from tests import _dense_cases as dc


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_bnbwd_chain_equals_autograd():
    """bnbwd_terms -> float64 finalize -> bnbwd_apply_ref = autograd through batch_norm(training) + relu"""
    M, C, eps = 37, 16, 1e-3
    g = _gen(1)
    z = torch.randn((M, C), generator=g, dtype=torch.float64) * 2
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    gamma[::4] *= -1
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    dh = torch.randn((M, C), generator=g, dtype=torch.float64)
    zr, gr, br = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.relu(F.batch_norm(zr, None, None, gr, br, training=True, eps=eps)).backward(dh)
    mean, inv = z.mean(0), (z.var(0, unbiased=False) + eps).rsqrt()
    bn = torch.cat([gamma * inv, beta, mean, inv])
    dm, dmx = dc.bnbwd_terms(dh, z, bn)
    bnb, dgamma, dbeta = dc.bnbwd_finalize_ref(dm.sum(0), dmx.sum(0), M, gamma, bn)
    dz, _ = dc.bnbwd_apply_ref(dh, z, bn, bnb.flatten())
    for got, want in ((dz, zr.grad), (dgamma, gr.grad), (dbeta, br.grad)):
        assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    assert (dm == 0).any() and (dm != 0).any()


def test_bn_apply_ref_equals_torch():
    g = _gen(2)
    bn = dc.bn_vec(24, g)
    z = dc.decisive_z(19, bn, g)
    sc, be, mu, _ = bn.double().view(4, -1)
    ref, mag = dc.bn_apply_ref(z, bn)
    assert torch.equal(ref, torch.relu((z.double() - mu) * sc + be))
    assert (mag >= ref).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pack_round_trips(dtype):
    img = torch.randn((5, 16), generator=_gen(3)).to(dtype)
    buf = dc.pack(img, 40, 24, spare=3)
    assert buf.shape == (8, 40) and buf.dtype == dtype
    assert torch.equal(dc.unpack(buf, 5, 16, 24).view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       img.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    assert dc.outside_unchanged(buf, 5, 16, 24)
    assert int(dc.is_sentinel(buf).sum()) == 8 * 40 - 5 * 16
    for r, c in ((0, 23), (4, 0), (5, 24), (7, 39)):             # one changed element outside is noticed
        b2 = buf.clone()
        b2[r, c] = 1.0
        assert not dc.outside_unchanged(b2, 5, 16, 24)
    b2 = buf.clone()
    b2[2, 30] = 0.0                                              # inside: not its business
    assert dc.outside_unchanged(b2, 5, 16, 24)


@pytest.mark.parametrize("fmap", [dc.S1, dc.S2, dc.D2, dc.P1, dc.U2, dc.G2, dc.FS1])
def test_conv_ref_equals_gather_loop(fmap):
    """one 5x4 row image per map (S2 / D2 also against an odd-sized partner)"""
    cin, cout = 3, 5
    cases = [dc.geometry(fmap, (2, 5, 4))]
    if fmap == dc.S2:
        cases.append(((2, 5, 4), (2, 9, 7), (2, 5, 4)))
    if fmap == dc.D2:
        cases.append(((2, 9, 7), (2, 5, 4), (2, 9, 7)))
    for R, S, O in cases:
        g = _gen(fmap)
        x = torch.randn((dc.npix(S), cin), generator=g, dtype=torch.float64)
        W = torch.randn(dc.layer_weight_shape(fmap, cin, cout), generator=g, dtype=torch.float64)
        ref, mag = dc.conv_ref(fmap, x, W, dc.KIND[fmap], R, S, O)
        want = dc.gather_conv(fmap, x, W, R, S, O)
        assert ref.shape == (dc.npix(O), cout)
        assert (ref - want).abs().max() <= 1e-12 * want.abs().max()
        magw = dc.gather_conv(fmap, x.abs(), W.abs(), R, S, O)
        assert (mag - magw).abs().max() <= 1e-12 * magw.abs().max()
        assert (mag >= ref.abs() - 1e-12).all()


@pytest.mark.parametrize("fmap", [dc.S1, dc.S2, dc.P1, dc.U2])
def test_wgrad_ref_equals_gather_loop(fmap):
    ci, co = 3, 4
    R, S, O = dc.geometry(fmap, (2, 5, 4)) if fmap != dc.S2 else ((2, 5, 4), (2, 9, 7), (2, 5, 4))
    g = _gen(20 + fmap)
    x = torch.randn((dc.npix(S), ci), generator=g, dtype=torch.float64)
    dz = torch.randn((dc.npix(O), co), generator=g, dtype=torch.float64)
    kind = dc.KIND[fmap]
    dW, mag = dc.wgrad_ref(fmap, x, dz, kind, R, S, O)
    T = dc.WTAPS[fmap]
    want = torch.zeros((T, ci, co), dtype=torch.float64)        # dW[t][ci][co] = sum_rows x[src] dz[row]
    sr = dc.src_rows(fmap, R, S)
    for t in range(T):
        for m in range(dc.npix(R)):
            if fmap == dc.U2:
                want[t] += torch.outer(x[m], dz[dc.out_rows(R, O, t)[m]])
            elif sr[m, t] >= 0:
                want[t] += torch.outer(x[sr[m, t]], dz[m])
    got = dW.reshape(dW.shape[0], dW.shape[1], T)
    got = got.permute(2, 1, 0) if kind == 0 else got.permute(2, 0, 1)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    assert (mag >= dW.abs() - 1e-12).all()
    nt = dc.tap_counts(fmap, R, S)
    assert nt.shape == (T,) and nt.max() <= dc.npix(R) and nt.min() >= 1


def test_margin_generator_on_every_case():
    for dtype in (torch.float32, torch.bfloat16):
        for C, M in dc.bn_shapes():
            g = _gen(C * 7 + M)
            bn = dc.bn_vec(C, g)
            z = dc.decisive_z(M, bn, g, dtype)
            assert z.dtype == dtype and z.shape == (M, C)
            pre = dc.pre_ref(z, bn)
            assert int((pre.abs() < 1e-3).sum()) == 0
            if M >= 255:
                assert (pre > 0).any() and (pre < 0).any()


def test_bf16_ties_are_ties():
    t = dc.bf16_ties(64, _gen(5))
    lo = (t.view(torch.int32) & ~0xFFFF).view(torch.float32)
    hi = ((t.view(torch.int32) & ~0xFFFF) + 0x10000).view(torch.float32)
    assert torch.equal((lo.double() + hi.double()) / 2, t.double())
    r = t.to(torch.bfloat16).float()
    assert ((r == lo) | (r == hi)).all() and (r == lo).any() and (r == hi).any()
