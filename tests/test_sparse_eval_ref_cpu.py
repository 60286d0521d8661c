"""Pins tests/_sparse_eval_ref.py (the float64 eval-mode SparseEncoder the GPU eval tests compare against) to the
train-mode oracle: with every layer's running statistics set to that layer's batch mean and biased variance,
running-statistics BatchNorm is batch-statistics BatchNorm, so the two dense outputs must agree to rounding."""
import pytest
import torch

from oracle.sparse_encoder import OracleSparseEncoder
from robustpointclouds_amd.sparse_encoder import SparseEncoder
from tests._sparse_eval_ref import BASIC, SPARSE_SHAPE, EvalSparseRef, frames_input, randomize_bn


@pytest.mark.parametrize("basic", [False, True])
def test_eval_reference_equals_train_oracle_on_batch_statistics(basic):
    torch.manual_seed(0)
    feats, coors = frames_input([0, 1], stride=8, extra_feature=basic)
    enc = SparseEncoder(feats.shape[1], SPARSE_SHAPE, **(BASIC if basic else {}))
    randomize_bn(enc)
    orc = OracleSparseEncoder(enc)
    want = orc.forward(feats, coors, 2, keep=True).detach()   # keep: the per-layer trace (c_out, z, pre)
    stats = [(z.detach().mean(0), z.detach().var(0, unbiased=False)) for _, z, _ in orc.trace]
    got = EvalSparseRef(enc, stats=stats).forward(feats, coors, 2)
    assert got.shape == want.shape == (2, 256, 200, 176)
    assert float(want.abs().max()) > 0.1
    err = float((got - want).abs().max())
    print("eval reference vs train oracle on its own batch statistics: max |diff|", err)
    assert err <= 1e-12
    # and it is an eval-mode encoder: the module's own running statistics give something else
    other = EvalSparseRef(enc).forward(feats, coors, 2)
    assert float((other - want).abs().max()) > 1e-3
