"""Attacked evaluation (AdversarialVoxelNet.attack_eval): the gate of extract_feat in eval mode, on the CPU.

The detector is the stand-in of tests/test_adversarial_voxelnet.py (built locally) with the CPU oracle perturber
in the adversary slot, so the explicit compaction path of extract_feat runs; the adversary module follows its own
`training` flag like the real VoxelPerturber (eval: running-statistics BatchNorm and eval bounds). The HIP
perturber and the fused path are covered by tests/test_gpu_predict_eval.py."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import robustpointclouds_amd.plugin.models  # noqa: F401  (registers the plugin types)
from oracle.perturber import OraclePerturber, perturb_voxels
from robustpointclouds_amd.plugin.models.detectors.adversarial_voxelnet import AdversarialVoxelNet
from tests.conftest import GOLDEN

TOL = 1e-4   # the perturber's parity bar


class RecordingVFE(nn.Module):
    """HardSimpleVFE semantics; keeps the voxels it was given."""

    def forward(self, features, num_points, coors):
        self.seen = features.detach().clone()
        return features[:, :, :4].sum(dim=1) / num_points.type_as(features).view(-1, 1)


class Middle(nn.Module):
    def forward(self, feats, coors, batch_size):
        out = feats.new_zeros(batch_size, feats.shape[1])
        return out.index_add(0, coors[:, 0].long(), feats.to(out.dtype))


class Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(4, 3))


class OracleAdversary(nn.Module):
    """The CPU oracle perturber in the adversary slot, in the mode of its own `training` flag."""

    def __init__(self, op):
        super().__init__()
        self.op = op

    def forward(self, x):
        out, ld = self.op.forward(x, training=self.training)
        return out.to(x.dtype), ld


def _oracle(d):
    op = OraclePerturber(d, 4, [int(h) for h in d["hidden"]])
    g = torch.Generator().manual_seed(11)   # running statistics unlike the batch's, and unlike the initial 0 / 1
    op.rm = [torch.rand(t.shape, generator=g, dtype=torch.float64) * 0.2 - 0.1 for t in op.rm]
    op.rv = [torch.rand(t.shape, generator=g, dtype=torch.float64) * 1.5 + 0.5 for t in op.rv]
    return op


@pytest.fixture()
def setup():
    d = dict(np.load(os.path.join(GOLDEN, "voxelnet_list_e3.npz")))
    m = AdversarialVoxelNet(adversary_cfg=dict(type="VoxelPerturber", hidden_channels=[int(h) for h in d["hidden"]]),
                            voxel_encoder=RecordingVFE(), middle_encoder=Middle(), backbone=nn.Identity(), neck=None,
                            bbox_head=Head())
    m.adversary = OracleAdversary(_oracle(d))
    m._epoch = 3
    m.eval()
    inputs = {"voxels": {"voxels": torch.from_numpy(d["vox"]), "num_points": torch.from_numpy(d["num_points"]),
                         "coors": torch.from_numpy(d["coors"])}, "batch_size": 2}
    _, want, ld = perturb_voxels(_oracle(d), d["vox"], d["num_points"], training=False)
    return m, inputs, d, want.detach(), float(ld["l2_norm"].detach())


def _close(got, want):
    return float((got.double() - want).abs().max()) <= TOL * max(1.0, float(want.abs().max()))


def test_clean_eval_leaves_voxels_alone(setup):
    m, inputs, d, want, l2 = setup
    with torch.no_grad():
        m.extract_feat(inputs)
    assert torch.equal(m.voxel_encoder.seen, torch.from_numpy(d["vox"]))
    assert m._current_l2_norm is None


def test_attack_eval_runs_the_eval_perturber(setup):
    m, inputs, d, want, l2 = setup
    assert float((want - torch.from_numpy(d["vox"]).double()).abs().max()) > 1e-3   # the attack moves the points
    with torch.no_grad(), m.attack_eval():
        m.extract_feat(inputs)
    assert _close(m.voxel_encoder.seen, want)
    assert abs(float(m._current_l2_norm) - l2) <= TOL * max(1.0, l2)
    # it was the eval forward: the train-mode perturber (batch statistics, training bounds) gives other voxels
    _, train, _ = perturb_voxels(_oracle(d), d["vox"], d["num_points"], training=True)
    assert not _close(m.voxel_encoder.seen, train.detach())
    # outside the block the gate is closed again
    with torch.no_grad():
        m.extract_feat(inputs)
    assert m._current_l2_norm is None and torch.equal(m.voxel_encoder.seen, torch.from_numpy(d["vox"]))


def test_attack_eval_keeps_the_epoch_gate(setup):
    m, inputs, d, want, l2 = setup
    m._epoch = 2
    with torch.no_grad(), m.attack_eval():
        m.extract_feat(inputs)
    assert m._current_l2_norm is None
    assert torch.equal(m.voxel_encoder.seen, torch.from_numpy(d["vox"]))


def test_attack_eval_ignores_adversarial_disabled(setup):
    m, inputs, d, want, l2 = setup
    m._adversarial_disabled = True
    with torch.no_grad(), m.attack_eval():
        m.extract_feat(inputs)
    assert _close(m.voxel_encoder.seen, want)
    assert m._adversarial_disabled is True
    with torch.no_grad():   # and outside the block the flag counts as before
        m.train()
        m.extract_feat(inputs)
    assert m._current_l2_norm is None


def test_attack_eval_restores_state(setup):
    m, inputs, d, want, l2 = setup
    modes = {n: mod.training for n, mod in m.named_modules()}
    assert not any(modes.values()) and m._attack_eval is False
    with m.attack_eval():
        assert m._attack_eval is True
        assert {n: mod.training for n, mod in m.named_modules()} == modes
    assert m._attack_eval is False
    with pytest.raises(ZeroDivisionError):
        with m.attack_eval():
            1 / 0
    assert m._attack_eval is False
    assert {n: mod.training for n, mod in m.named_modules()} == modes
    with m.attack_eval():      # nested blocks restore the enclosing state
        with m.attack_eval():
            pass
        assert m._attack_eval is True
    assert m._attack_eval is False
