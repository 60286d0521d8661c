"""The perturber's option matrix and edge shapes (csrc/perturber.hip) against the float64 CPU oracle: every
kernel family x attention on / off x point counts below, at and next to the 64-point group and 256-thread
block edges; eval mode after a train step; the plugin's zero-padding at a tail; fused voxels with any slots /
vfe_features / eval; the fallbacks (no valid point, one valid point); 16-bit rows without the split weight
gradient and at tails. Cases, inputs, runners and bounds: tests/_perturber_cases.py (the bounds are those of
tests/test_gpu_perturber.py); tests/test_perturber_matrix_inputs.py checks on the CPU that the inputs are fair."""
import numpy as np
import pytest
import torch

from robustpointclouds_amd import perturb as P
from tests import _perturber_cases as M

pytestmark = pytest.mark.gpu


# Both settings of rpc_perturber_cfg.double_sums run every case against the same oracle and the same bounds: "double"
# is parity mode (make_cfg's default), "float" the bf16 trainer's and the benchmark's float batch sums.
SUMS = pytest.mark.parametrize("double_sums", [True, False], ids=["double", "float"])


# ------------------------------------------------------------------ standalone matrix
@SUMS
@pytest.mark.parametrize("case", M.STANDALONE + [M.LARGE + (True,)], ids=M.sid)
def test_standalone_train_matches_oracle(case, double_sums):
    """Float sums meet every bound but in the two cases of M.FLOAT_SUMS_CASES, both with two points. There the
    bound grows by what M.float_sums_allowance derives from float32's roundoff and the float64 oracle, and by no
    more. Measured with float sums: 64-128-64_F4_N2_noatt imbalance loss 1.3e-5 off (allowance 1.5e-4);
    64-128-64_F4_N2_att dW0 / dW1 / dW2 4.1e-3 / 3.9e-3 / 4.7e-3 of their max-abs (2e-3 + 3.7e-3 / 2.2e-3 / 3.6e-3)."""
    inp = M.standalone_inputs(case)
    got = M.run_hip_standalone(case, inp, double_sums=double_sums)
    assert got["flags"][5] == 0.0 and got["flags"][4] == case[2]
    for k in M.ATT_SLOTS:      # no attention: four null parameter pointers, no gradient for them
        assert (got["grad_slots"][k] is None) == (not case[3]), k
    ref = M.run_oracle_standalone(case, inp)
    imb_atol, grad_extra = (0.0, None)
    if not double_sums and case in M.FLOAT_SUMS_CASES:
        imb_atol, grad_extra = M.float_sums_allowance(case, inp, ref)
    M.compare(got, ref, imb_atol=imb_atol, grad_extra=grad_extra)


@SUMS
@pytest.mark.parametrize("case", M.EVAL, ids=M.sid)
def test_standalone_eval_after_train_step_matches_oracle(case, double_sums):
    inp = M.standalone_inputs(case, eval_half=True)
    got = M.run_hip_standalone(case, inp, backward=False, double_sums=double_sums)
    ref = M.run_oracle_standalone(case, inp, backward=False)
    np.testing.assert_allclose(got["out_eval"], ref["out_eval"], rtol=0, atol=M.TOL)
    np.testing.assert_allclose(got["l2_eval"], ref["l2_eval"], rtol=M.LOSS_RTOL)


def test_plugin_padding_at_tail_matches_oracle():
    """[12, 24, 40] runs zero-padded to [16, 32, 64]; N = 65 leaves one point in the second 64-point group.
    Assertions as in test_plugin_arbitrary_widths_match_oracle, attention off."""
    hidden, F, N = M.PLUGIN_TAIL
    dev = torch.device("cuda")
    vp, w = M.plugin_perturber(M.seed_of("plugin", *M.PLUGIN_TAIL), hidden, False)
    vp = vp.to(dev).train()
    assert vp._padded() and vp.attention is None
    case = (hidden, F, N, False)
    inp = dict(M.standalone_inputs(case), w=w)
    out, ld = vp(torch.from_numpy(inp["x"]).to(dev))
    (out * torch.from_numpy(inp["G"]).to(dev)).sum().add(sum(ld[k] * float(M.CL[i]) for i, k in enumerate(M.LOSS_KEYS))
                                                         ).backward()
    bns = [m for m in vp.model if isinstance(m, torch.nn.BatchNorm1d)]
    got = dict(out=out.detach().cpu().numpy(), lvec=np.array([float(ld[k]) for k in M.LOSS_KEYS]),
               grads=M.plugin_grads(vp), rm=[m.running_mean.cpu().numpy() for m in bns],
               rv=[m.running_var.cpu().numpy() for m in bns])
    M.compare(got, M.run_oracle_standalone(case, inp))


# ------------------------------------------------------------------ fused matrix
@SUMS
@pytest.mark.parametrize("case", M.FUSED, ids=M.fid)
def test_fused_matches_oracle(case, double_sums):
    """(3, 70, ...) is the only case whose rows span a whole wave in k_valid_count_pts (slots >= 64)."""
    inp = M.fused_inputs(case)
    got = M.run_hip_fused(case, inp, double_sums=double_sums)
    assert got["flags"][5] == 0.0
    M.compare(got, M.run_oracle_fused(case, inp))


# ------------------------------------------------------------------ fallbacks
def _fallback_voxels(one_point):
    V, slots, F = 40, 5, 4
    vox = np.zeros((V, slots, F), np.float32)
    if one_point:
        vox[17, 0] = [12.5, -3.25, 0.5, 0.21]
    return vox, np.ones(V, np.int32)


@pytest.mark.parametrize("one_point", [False, True], ids=["all_zero", "one_valid_point"])
def test_fused_train_fallback_below_two_points(one_point):
    """No valid point: the reference skips the adversary (adversarial_voxelnet.py:118-121). One valid point: its
    train-mode BatchNorm1d raises ("Expected more than 1 value per channel") before any running statistic is
    touched, and the detector falls back to the unperturbed voxels with zero losses (:123-132). Either way:
    the flag, the input voxels bit for bit, zero losses, the plain voxel mean, zero gradients and untouched
    running statistics."""
    dev = torch.device("cuda")
    hidden, F, vf = (8, 16, 32), 4, 4
    vox, npts = _fallback_voxels(one_point)
    w = M.make_weights(M.seed_of("fallback", one_point), F, hidden, True, running=True)
    ps = M.hip_params(w, F, hidden, dev)
    vt, nt = torch.from_numpy(vox).to(dev), torch.from_numpy(npts).to(dev)
    vfe, lvec, pert, flags = P.PerturbVoxelsFn.apply(vt, nt, P.make_cfg(F, list(hidden), True, True, 0.2, vfe_features=vf),
                                                    *ps)
    assert flags[5].item() == 1.0 and flags[4].item() == float(one_point)
    assert np.array_equal(pert.cpu().numpy().view(np.uint32), vox.view(np.uint32))
    assert np.all(lvec.detach().cpu().numpy() == 0)
    mean = P.VoxelMeanFn.apply(vt, nt, vf)
    assert np.array_equal(vfe.detach().cpu().numpy().view(np.uint32), mean.cpu().numpy().view(np.uint32))
    for t in (vfe, lvec, pert, flags):
        assert bool(torch.isfinite(t).all())
    G = M.make_upstream(3, (vox.shape[0], vf))
    ((vfe * torch.from_numpy(G).to(dev)).sum() + (lvec * torch.from_numpy(M.CL).to(dev)).sum()).backward()
    for k, name in enumerate(M.NAMES):
        if name is None:
            want = w[f"r{'m' if k % 6 == 4 else 'v'}{k // 6}"]
            assert np.array_equal(ps[k].cpu().numpy().view(np.uint32), want.view(np.uint32)), (k, "running stat")
        else:
            assert ps[k].grad is not None and bool((ps[k].grad == 0).all()), name


# ------------------------------------------------------------------ 16-bit rows
def _a16_case(shape, n):
    return (shape[0], shape[1], n, True)


_shape_id = lambda s: "-".join(map(str, s[0]))


@pytest.mark.parametrize("act16", [1, 3])
@pytest.mark.parametrize("shape", M.A16_SHAPES, ids=_shape_id)
def test_act16_without_split_is_fp32_rows(shape, act16):
    """16-bit rows exist only together with the split-bf16 weight gradient (fill_dev): the fp32-MFMA k_wgrad_mf
    reads its rows as fp32, so act16 without wgrad_split_bf16 must run exactly the act16 = 0 step. Fails on any
    build where fp16 z rows reach k_wgrad_mf (the hidden-layer weight gradients are then garbage)."""
    case = _a16_case(shape, 2500)
    inp = M.standalone_inputs(case)
    a = M.run_hip_standalone(case, inp, split=False, act16=0)
    b = M.run_hip_standalone(case, inp, split=False, act16=act16)
    bits = lambda t: np.ascontiguousarray(t).view(np.uint32)
    for k in ("out", "lvec"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for k in ("rm", "rv"):
        for l in range(5):
            assert np.array_equal(bits(a[k][l]), bits(b[k][l])), (k, l)
    assert a["grads"].keys() == b["grads"].keys()
    for name in a["grads"]:
        assert np.array_equal(bits(a["grads"][name]), bits(b["grads"][name])), name


@pytest.mark.parametrize("n", M.A16_TAILS)
@pytest.mark.parametrize("act16", [1, 2, 3])
@pytest.mark.parametrize("shape", M.A16_SHAPES, ids=_shape_id)
def test_act16_tails_close_to_fp32(shape, act16, n):
    """The 16-bit ldq / stq load whole vectors and mask by n + i < N: one point past a 64-point group and past a
    256-point block, split-bf16 weight gradients both ways. Every output and gradient finite; rel(out - x) and the
    loss terms within the 5e-3 of test_act16_rows_close_to_fp32 of the fp32-rows run on the same input. The
    gradients are not bounded: that test's gradient bounds are statistical in N and do not transfer."""
    case = _a16_case(shape, n)
    inp = M.standalone_inputs(case)
    ref = M.run_hip_standalone(case, inp, split=True, act16=0)
    got = M.run_hip_standalone(case, inp, split=True, act16=act16)
    for k in ("out", "lvec", "flags"):
        assert np.isfinite(got[k]).all(), k
    for k in ("rm", "rv"):
        assert all(np.isfinite(t).all() for t in got[k]), k
    for name, g in got["grads"].items():
        assert np.isfinite(g).all(), name
    assert got["flags"][5] == 0.0
    ep, el = M.a16_errors(got, ref, inp["x"].astype(np.float64))
    print(f"act16={act16} N={n} {_shape_id(shape)}: perturbation rel {ep:.2e}, losses rel {el:.2e}")
    assert ep <= M.A16_TOL and el <= M.A16_TOL, (ep, el)
