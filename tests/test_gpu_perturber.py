"""a2–a5 parity: the HIP perturber (+ fused compaction / scatter / VFE) against the golden
vectors of the reference VoxelPerturber and against the CPU oracle."""
import os

import numpy as np
import pytest
import torch

from oracle.perturber import OraclePerturber, perturb_voxels
from robustpointclouds_amd import perturb as P
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
TOL = 1e-4   # north_star: perturbed coords and losses within 1e-4 (fp32)


def _params(d, F, hidden, dev, att=True):
    """36 tensors in rpc_perturber order (include/rpc_hip.h)."""
    widths = [F, hidden[0], hidden[1], hidden[2], hidden[1], hidden[0]]
    t = lambda k: torch.tensor(np.asarray(d[k]), dtype=torch.float32, device=dev).contiguous()
    ps = []
    for l in range(5):
        ps += [t(f"W{l}"), t(f"b{l}"), t(f"g{l}"), t(f"be{l}"),
               torch.zeros(widths[l + 1], device=dev), torch.ones(widths[l + 1], device=dev)]
    ps += [t("W5"), t("b5")]
    ps += [t("Wa0"), t("ba0"), t("Wa1"), t("ba1")] if att else [None] * 4
    return ps


def _load(tag):
    return dict(np.load(os.path.join(GOLDEN, f"perturber_{tag}.npz")))


NAMES = []
for _l in range(5):
    NAMES += [f"W{_l}", f"b{_l}", f"g{_l}", f"be{_l}", None, None]
NAMES += ["W5", "b5", "Wa0", "ba0", "Wa1", "ba1"]


@pytest.mark.parametrize("tag", ["car_small", "car_clamp", "3class", "nus"])
def test_standalone_matches_reference_golden(tag):
    _standalone_golden(tag, True)


@pytest.mark.parametrize("tag", ["car_small", "car_clamp", "3class", "nus"])
def test_standalone_float_sums_match_reference_golden(tag):
    """The bf16 trainer's float batch sums (rpc_perturber_cfg.double_sums = 0, what the benchmark runs) against the
    same golden vectors and the same bounds."""
    _standalone_golden(tag, False)


def _standalone_golden(tag, double_sums):
    d = _load(tag)
    F, hidden = int(d["F"]), [int(h) for h in d["hidden"]]
    dev = torch.device("cuda")
    ps = _params(d, F, hidden, dev)
    for p in ps:
        if p is not None:
            p.requires_grad_(True)
    for l in range(5):
        ps[6 * l + 4].requires_grad_(False)
        ps[6 * l + 5].requires_grad_(False)
    cfg = P.make_cfg(F, hidden, True, True, 0.2, double_sums=double_sums)
    x = torch.from_numpy(d["x"]).to(dev)
    out, lvec, flags = P.PerturberFn.apply(x, cfg, *ps)
    np.testing.assert_allclose(out.detach().cpu().numpy(), d["out"], rtol=0, atol=TOL)
    got = lvec.detach().cpu().numpy()
    ref = np.array([d["l2_norm"], d["intensity_loss"], d["bias_loss"], d["imbalance_loss"]])
    np.testing.assert_allclose(got, ref, rtol=TOL, atol=1e-6)
    G = torch.from_numpy(d["G"]).to(dev)
    c = torch.from_numpy(d["c"]).to(dev)
    loss = (out * G).sum() + (lvec * c).sum()
    loss.backward()
    for k, name in enumerate(NAMES):
        if name is None:
            continue
        g = ps[k].grad.cpu().numpy()
        r = d["d" + name]
        scale = max(np.abs(r).max(), 1e-3)
        tol = 1e-3
        if name[0] == "b" and name[1:].isdigit() and int(name[1:]) < 5:
            # bias of a Linear feeding a train-mode BatchNorm: the exact gradient is 0 (BN removes
            # any constant); reference and kernel both return fp32 cancellation noise, whose pattern
            # follows the summation order -> bounded by 1e-2 of the layer's dW scale
            scale = max(scale, np.abs(d["dW" + name[1:]]).max())
            tol = 1e-2
        np.testing.assert_allclose(g, r, rtol=0, atol=tol * scale, err_msg=name)
    for l in range(5):
        np.testing.assert_allclose(ps[6 * l + 4].cpu().numpy(), d[f"rm{l}"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(ps[6 * l + 5].cpu().numpy(), d[f"rv{l}"], rtol=1e-4, atol=1e-5)
    # eval mode with the updated running stats
    cfg_e = P.make_cfg(F, hidden, True, False, 0.2, double_sums=double_sums)
    with torch.no_grad():
        oute, lve, _ = P.PerturberFn.apply(torch.from_numpy(d["x_eval"]).to(dev), cfg_e, *ps)
    np.testing.assert_allclose(oute.cpu().numpy(), d["out_eval"], rtol=0, atol=TOL)
    np.testing.assert_allclose(lve[0].item(), float(d["l2_norm_eval"]), rtol=TOL)


def _voxels(seed, V, x_pool):
    rng = np.random.default_rng(seed)
    F = x_pool.shape[1]
    vox = np.zeros((V, 5, F), np.float32)
    npts = rng.choice([1, 1, 1, 1, 2, 2, 3, 4, 5], V).astype(np.int32)
    for v in range(V):
        vox[v, :npts[v]] = x_pool[rng.integers(0, len(x_pool), npts[v])]
    vox[5, 0] = [1.0, -1.0] + [0.0] * (F - 2)     # real point with zero feature sum (reference: padding)
    return vox, npts


@pytest.mark.parametrize("tag,V", [("car_small", 3000), ("3class", 1500), ("car_small", 70000), ("nus", 3000)])
def test_fused_voxels_vfe_matches_oracle(tag, V):
    """nus: F = 5 (x, y, z, intensity, time lag) with HardSimpleVFE(num_features=5), CenterPoint's path."""
    _fused_vfe(tag, V, True)


@pytest.mark.parametrize("tag,V", [("car_small", 3000), ("3class", 1500), ("car_small", 70000), ("nus", 3000)])
def test_fused_voxels_vfe_float_sums_match_oracle(tag, V):
    """The bf16 trainer's float batch sums (rpc_perturber_cfg.double_sums = 0) on the fused path, same bounds."""
    _fused_vfe(tag, V, False)


def _fused_vfe(tag, V, double_sums):
    d = _load(tag)
    hidden = [int(h) for h in d["hidden"]]
    F = d["x"].shape[1]
    dev = torch.device("cuda")
    vox, npts = _voxels(1, V, d["x"])
    ps = _params(d, F, hidden, dev)
    for p in ps:
        if p is not None:
            p.requires_grad_(True)
    for l in range(5):
        ps[6 * l + 4].requires_grad_(False)
        ps[6 * l + 5].requires_grad_(False)
    cfg = P.make_cfg(F, hidden, True, True, 0.2, vfe_features=F, double_sums=double_sums)
    vt, nt = torch.from_numpy(vox).to(dev), torch.from_numpy(npts).to(dev)
    vfe, lvec, pert, flags = P.PerturbVoxelsFn.apply(vt, nt, cfg, *ps)
    op = OraclePerturber(d, F, hidden, dtype=torch.float64)
    rvfe, rpert, rld = perturb_voxels(op, vox, npts, vfe_features=F)
    np.testing.assert_allclose(pert.cpu().numpy(), rpert.detach().numpy(), rtol=0, atol=TOL)
    np.testing.assert_allclose(vfe.detach().cpu().numpy(), rvfe.detach().numpy(), rtol=0, atol=TOL)
    ref = torch.stack([rld[k] for k in ["l2_norm", "intensity_loss", "bias_loss", "imbalance_loss"]])
    np.testing.assert_allclose(lvec.detach().cpu().numpy(), ref.detach().numpy(), rtol=TOL, atol=1e-6)
    assert int(flags[4].item()) == int((vox.reshape(-1, F).sum(1) != 0).sum())
    # backward through the fused VFE
    rng = np.random.default_rng(2)
    Gv = rng.standard_normal((V, F)).astype(np.float32) * 1e-3
    cl = np.array([1e-3, -2e-3, 3e-3, 1e-3], np.float32)
    ((vfe * torch.from_numpy(Gv).to(dev)).sum() + (lvec * torch.from_numpy(cl).to(dev)).sum()).backward()
    rloss = (rvfe * torch.from_numpy(Gv.astype(np.float64))).sum() + (ref * torch.from_numpy(cl.astype(np.float64))).sum()
    rloss.backward()
    rg = op.grads()
    for k, name in enumerate(NAMES):
        if name is None:
            continue
        g = ps[k].grad.cpu().numpy()
        r = rg["d" + name].numpy()
        scale = max(np.abs(r).max(), 1e-6)
        if name[0] == "b" and name[1:].isdigit() and int(name[1:]) < 5:
            assert np.abs(g).max() <= 1e-3 * max(np.abs(rg["dW" + name[1:]].numpy()).max(), 1e-6) + 1e-9
            continue
        np.testing.assert_allclose(g, r, rtol=0, atol=2e-3 * scale, err_msg=name)


def test_fused_is_deterministic():
    d = _load("car_small")
    dev = torch.device("cuda")
    vox, npts = _voxels(3, 20000, d["x"])
    outs = []
    for _ in range(2):
        ps = _params(d, 4, [8, 16, 32], dev)
        cfg = P.make_cfg(4, [8, 16, 32], True, True, 0.2)
        vfe, lvec, pert, _ = P.PerturbVoxelsFn.apply(torch.from_numpy(vox).to(dev), torch.from_numpy(npts).to(dev),
                                                    cfg, *ps)
        outs.append((vfe.cpu().numpy(), lvec.cpu().numpy(), pert.cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_nan_input_falls_back_to_unperturbed():
    d = _load("car_small")
    dev = torch.device("cuda")
    vox, npts = _voxels(4, 500, d["x"])
    vox[10, 0, 2] = np.nan
    ps = _params(d, 4, [8, 16, 32], dev)
    cfg = P.make_cfg(4, [8, 16, 32], True, True, 0.2)
    vfe, lvec, pert, flags = P.PerturbVoxelsFn.apply(torch.from_numpy(vox).to(dev), torch.from_numpy(npts).to(dev),
                                                    cfg, *ps)
    assert flags[5].item() == 1.0
    assert np.array_equal(pert.cpu().numpy(), vox, equal_nan=True)
    assert np.all(lvec.cpu().numpy() == 0)


def test_vfe_mean_bit_exact():
    rng = np.random.default_rng(0)
    V = 5000
    vox = rng.standard_normal((V, 5, 4)).astype(np.float32)
    npts = rng.integers(1, 6, V).astype(np.int32)
    out = P.VoxelMeanFn.apply(torch.from_numpy(vox).cuda(), torch.from_numpy(npts).cuda(), 4).cpu().numpy()
    ref = (torch.from_numpy(vox)[:, :, :4].sum(dim=1) / torch.from_numpy(npts).float().view(-1, 1)).numpy()
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("hidden", [[12, 24, 40], [8, 100, 20], [64, 128, 256, 128], [40, 200, 130]])
def test_plugin_arbitrary_widths_match_oracle(hidden):
    """The reference builds any hidden_channels (voxel_perturber.py:82-103); non-native widths run
    zero-padded to the kernel widths. Forward, loss terms, every parameter gradient (after the
    ±0.1 hook clamp) and the BatchNorm running statistics must match the float64 oracle.
    [64, 128, 256, 128] is configs/adversarial/adversarial-second_strong_v2.py's list (the reference reads
    its first three entries): its 256-wide layers run on the per-point VALU kernels; [40, 200, 130] pads
    to [64, 256, 256]."""
    from robustpointclouds_amd.plugin.models.adversarial.voxel_perturber import VoxelPerturber
    dev = torch.device("cuda")
    torch.manual_seed(3)
    vp = VoxelPerturber(hidden_channels=hidden).to(dev).train()
    hidden = hidden[:3]
    assert vp._padded() == (hidden != [64, 128, 256])
    lin = [m for m in vp.model if isinstance(m, torch.nn.Linear)]
    bns = [m for m in vp.model if isinstance(m, torch.nn.BatchNorm1d)]
    att = [m for m in vp.attention if isinstance(m, torch.nn.Linear)]
    w = {}
    for l, m in enumerate(lin):
        w[f"W{l}"], w[f"b{l}"] = m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()
    for l, m in enumerate(bns):
        with torch.no_grad():     # non-trivial affine parameters
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.2, 0.2)
        w[f"g{l}"], w[f"be{l}"] = m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()
    for l, m in enumerate(att):
        w[f"Wa{l}"], w[f"ba{l}"] = m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()
    d = _load("3class")
    x = torch.from_numpy(d["x"]).to(dev)
    out, ld = vp(x)
    op = OraclePerturber(w, 4, hidden, dtype=torch.float64)
    rout, rld = op.forward(torch.from_numpy(d["x"]))
    np.testing.assert_allclose(out.detach().cpu().numpy(), rout.detach().numpy(), rtol=0, atol=TOL)
    for k in ("l2_norm", "intensity_loss", "bias_loss", "imbalance_loss"):
        np.testing.assert_allclose(float(ld[k]), float(rld[k]), rtol=TOL, atol=1e-7, err_msg=k)
    G = torch.from_numpy(d["G"])
    c = torch.from_numpy(d["c"])
    lk = ["l2_norm", "intensity_loss", "bias_loss", "imbalance_loss"]
    ((out * G.to(dev)).sum() + sum(ld[k] * float(c[i]) for i, k in enumerate(lk))).backward()
    ((rout * G.double()).sum() + sum(rld[k] * float(c[i]) for i, k in enumerate(lk))).backward()
    rg = op.grads()
    got = {}
    for l, m in enumerate(lin):
        got[f"W{l}"], got[f"b{l}"] = m.weight.grad, m.bias.grad
    for l, m in enumerate(bns):
        got[f"g{l}"], got[f"be{l}"] = m.weight.grad, m.bias.grad
    for l, m in enumerate(att):
        got[f"Wa{l}"], got[f"ba{l}"] = m.weight.grad, m.bias.grad
    for k, g in got.items():
        r = rg["d" + k].numpy()
        assert g.shape == r.shape, k
        if k[0] == "b" and k[1:].isdigit() and int(k[1:]) < 5:
            continue   # exact gradient 0 (a constant before train-mode BN): cancellation noise on both sides
        np.testing.assert_allclose(g.cpu().numpy(), r, rtol=0, atol=2e-3 * max(np.abs(r).max(), 1e-6), err_msg=k)
    for l, m in enumerate(bns):
        np.testing.assert_allclose(m.running_mean.cpu().numpy(), op.rm[l].numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(m.running_var.cpu().numpy(), op.rv[l].numpy(), rtol=1e-4, atol=1e-5)


def test_wgrad_split_bf16_close_to_fp32():
    """Perf mode's hidden-layer weight gradients on split-bf16 MFMA (hi/lo operands, k_wgrad_bx3) against
    the fp32-MFMA path on the same step (metric widths [64, 128, 64], 60k points): every gradient within
    relative L2 1e-4 (the dropped lo*lo term and bf16 hi/lo rounding: ~2^-16 per product); the other
    gradients, the forward and the loss terms unchanged bit for bit."""
    from robustpointclouds_amd.plugin.models.adversarial.voxel_perturber import VoxelPerturber
    dev = torch.device("cuda")
    torch.manual_seed(7)
    vp = VoxelPerturber(hidden_channels=[64, 128, 64]).to(dev).train()
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(60000, 4, generator=g) * torch.tensor([20.0, 20.0, 1.0, 0.3])).to(dev)
    G = (torch.randn(60000, 4, generator=g) * 1e-4).to(dev)
    res = {}
    for split in (False, True):
        vp.wgrad_split_bf16 = split
        vp.zero_grad(set_to_none=True)
        out, ld = vp(x)
        ((out * G).sum() + 1e-3 * ld["l2_norm"]).backward()
        torch.cuda.synchronize()
        res[split] = (out.detach().clone(), {n: p.grad.detach().clone() for n, p in vp.named_parameters()})
    assert torch.equal(res[False][0], res[True][0])
    lin = [n for n, m in vp.model.named_children() if isinstance(m, torch.nn.Linear)]
    mf = {f"model.{lin[l]}.weight" for l in range(1, 5)}
    # their biases feed train-mode BatchNorm: exact gradient 0, both paths give summation noise
    noise = {f"model.{lin[l]}.bias" for l in range(1, 5)}
    for n, a in res[False][1].items():
        b = res[True][1][n]
        if n in noise:
            continue
        if n in mf:
            rel = float((b - a).norm() / a.norm().clamp_min(1e-30))
            assert rel <= 1e-4, (n, rel)
        else:
            assert torch.equal(a, b), n


# (gradient rel-L2, cosine) bounds per act16: bf16 gradient rows alone round each term once (unbiased: sums keep
# ~2^-9 / sqrt(N)); fp16 pre-activations flip ReLU decisions (docstring). act16 = 1's 16-bit rows are a subset of
# act16 = 3's (the fp16 z rows without the bf16 gradient rows): it takes act16 = 3's entry
GRAD_BOUNDS = {1: (0.1, 0.995), 2: (1e-2, 0.9999), 3: (0.1, 0.995)}


@pytest.mark.parametrize("act16", [1, 2, 3])
def test_act16_rows_close_to_fp32(act16):
    """Perf mode's 16-bit hidden-layer rows (rpc_perturber_cfg.act16: 1 = fp16 pre-activations z_1..z_3, 2 = bf16
    gradient rows dh / dz, 3 = both; an option, off unless RPC_PERT_ACT16 is set: the bench's default is fp32 rows)
    against fp32 rows on the same step (metric widths [64, 128, 64], 60k points, split-bf16 weight gradients both ways). The reference AMP (train.py:91-103) runs these Linear layers in fp16.
    Bounds (measured r06 in the test output): perturbation (out - x) and the four loss terms within 5e-3 relative;
    every parameter gradient within GRAD_REL relative L2 and cosine >= GRAD_COS, the biases before train-mode
    BatchNorm excepted (exact gradient 0: summation noise). The gradient bound is loose by construction: with a
    random upstream gradient G the BatchNorm-beta / weight gradients are sums of zero-mean terms (~sqrt(N) of
    N), and every ReLU decision a 16-bit pre-activation takes differently (an fp16 rounding of z ~ 10 is ~5e-3
    of the normalised unit: ~0.2 % of the decisions) moves such a sum by a whole term — the same mechanism as
    the sparse encoder's (tests/test_gpu_sparse_layers.py). act16 = 1 (fp16 z rows, fp32 gradient rows) takes
    act16 = 3's bounds, its 16-bit rows being a subset; measured: perturbation 8.5e-4, losses 6.6e-6, worst gradient
    3.9e-2 relative (cosine 0.99926) — act16 = 3's figures (3.9e-2, 0.99925): the fp16 pre-activations, not the bf16
    gradient rows, set the gradient error. Training-level agreement is bounded by
    tests/test_gpu_bf16_trajectory.py on the real loss."""
    from robustpointclouds_amd.plugin.models.adversarial.voxel_perturber import VoxelPerturber
    dev = torch.device("cuda")
    torch.manual_seed(7)
    vp = VoxelPerturber(hidden_channels=[64, 128, 64]).to(dev).train()
    vp.wgrad_split_bf16 = True
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(60000, 4, generator=g) * torch.tensor([20.0, 20.0, 1.0, 0.3])).to(dev)
    G = (torch.randn(60000, 4, generator=g) * 1e-4).to(dev)
    res = {}
    for a in (0, act16):
        vp.act16 = a
        vp.zero_grad(set_to_none=True)
        out, ld = vp(x)
        ((out * G).sum() + 1e-3 * ld["l2_norm"]).backward()
        torch.cuda.synchronize()
        res[a] = (out.detach().clone(), {k: float(v) for k, v in ld.items()},
                  {n: p.grad.detach().clone() for n, p in vp.named_parameters()})
    (o0, l0, g0), (o1, l1, g1) = res[0], res[act16]
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
    ep = rel(o1 - x, o0 - x)
    el = max(abs(l1[k] - l0[k]) / max(abs(l0[k]), 1e-12) for k in l0)
    lin = [n for n, m in vp.model.named_children() if isinstance(m, torch.nn.Linear)]
    noise = {f"model.{lin[l]}.bias" for l in range(0, 5)}
    cos = lambda a, b: float((a.flatten() @ b.flatten()) / (a.norm() * b.norm()).clamp_min(1e-30))
    eg = sorted(((rel(g1[n], g0[n]), n, cos(g1[n], g0[n])) for n in g0 if n not in noise), reverse=True)
    print(f"act16={act16}: perturbation rel {ep:.2e}, losses rel {el:.2e}, worst gradients {eg[:4]}")
    assert ep <= 5e-3 and el <= 5e-3, (ep, el)
    grad_rel, grad_cos = GRAD_BOUNDS[act16]
    assert eg[0][0] <= grad_rel and min(e[2] for e in eg) >= grad_cos, eg[:4]
