"""CPU guard of the perturber option matrix (tests/_perturber_cases.py): a bound of the GPU tests is only fair
if the reference arithmetic itself stays inside it on the chosen inputs, and train-mode BatchNorm over a handful
of points is ill-conditioned. Every case's float32 oracle must agree with its float64 oracle within HALF the
bound tests/test_gpu_perturber_matrix.py applies to the kernels; the 16-bit tail cases likewise with a float64
oracle whose z_1..z_3 rows pass through fp16. A case that fails here gets another seed
(_perturber_cases.SEEDS), never a wider bound and never leaves the table."""
import numpy as np
import pytest
import torch

from oracle.perturber import OraclePerturber, bounds
from tests import _perturber_cases as M


# float32 evaluations per train case: the plain one and this many with the hidden channels renumbered. One
# evaluation is one sample of the float32 rounding; the worst of several is the fairer estimate of how far
# float32 arithmetic in another order (the kernels') can land from the float64 result.
RENUMBERINGS = (0, 1, 2, 3)


def test_renumbered_channels_are_the_same_network():
    case = ((16, 32, 64), 5, 65, True)
    inp = M.standalone_inputs(case)
    a, b = M.run_oracle_standalone(case, inp), M.run_oracle_standalone(case, inp, renumber=7)
    np.testing.assert_allclose(b["out"], a["out"], rtol=0, atol=1e-12)
    for k in a["grads"]:
        np.testing.assert_allclose(b["grads"][k], a["grads"][k], rtol=0, atol=1e-12 * max(np.abs(a["grads"][k]).max(), 1),
                                   err_msg=k)
    for l in range(5):
        np.testing.assert_allclose(b["rv"][l], a["rv"][l], rtol=1e-12)
        np.testing.assert_allclose(b["rm"][l], a["rm"][l], rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", M.STANDALONE + [M.LARGE + (True,)], ids=M.sid)
def test_standalone_train_inputs_well_conditioned(case):
    inp = M.standalone_inputs(case)
    ref = M.run_oracle_standalone(case, inp)
    for r in RENUMBERINGS if case[2] < 100000 else RENUMBERINGS[:2]:
        M.compare(M.run_oracle_standalone(case, inp, torch.float32, renumber=r), ref, frac=0.5)


@pytest.mark.parametrize("case", M.EVAL, ids=M.sid)
def test_standalone_eval_inputs_well_conditioned(case):
    inp = M.standalone_inputs(case, eval_half=True)
    a = M.run_oracle_standalone(case, inp, torch.float32, backward=False)
    b = M.run_oracle_standalone(case, inp, backward=False)
    np.testing.assert_allclose(a["out_eval"], b["out_eval"], rtol=0, atol=0.5 * M.TOL)
    np.testing.assert_allclose(a["l2_eval"], b["l2_eval"], rtol=0.5 * M.LOSS_RTOL)


@pytest.mark.parametrize("case", M.FUSED, ids=M.fid)
def test_fused_inputs_well_conditioned(case):
    inp = M.fused_inputs(case)
    assert inp["npts"].min() >= 1
    slot = np.arange(inp["vox"].shape[1])[None, :]
    assert np.all(inp["vox"][slot >= inp["npts"][:, None]] == 0)
    ref = M.run_oracle_fused(case, inp)
    assert 2 <= ref["nvalid"] < int(inp["npts"].sum())     # a real slot with zero feature sum is dropped
    M.compare(M.run_oracle_fused(case, inp, torch.float32), ref, frac=0.5)


def test_plugin_tail_inputs_well_conditioned():
    hidden, F, N = M.PLUGIN_TAIL
    _, w = M.plugin_perturber(M.seed_of("plugin", *M.PLUGIN_TAIL), hidden, False)
    case = (hidden, F, N, False)
    inp = dict(M.standalone_inputs(case), w=w)
    M.compare(M.run_oracle_standalone(case, inp, torch.float32), M.run_oracle_standalone(case, inp), frac=0.5)


class _Fp16RowsOracle(OraclePerturber):
    """OraclePerturber.forward with the pre-activations z_1..z_3 rounded through fp16 (act16 bit 0: the rows
    launch_mid16 keeps in fp16; BatchNorm then reads the stored row)."""
    row_dtype = torch.float16

    def forward(self, x, training=True):
        p = self.p
        x = torch.as_tensor(x).to(self.dtype)
        s = torch.std(x, dim=0, keepdim=True) + 1e-6
        if torch.isnan(s).any() or torch.isinf(s).any():
            s = torch.ones_like(s)
        xn = torch.clamp(x / s, -10.0, 10.0)
        h = xn
        for l in range(5):
            z = h @ p[f"W{l}"].T + p[f"b{l}"]
            if 1 <= l <= 3 and self.row_dtype is not None:
                z = z.to(self.row_dtype).to(self.dtype)
            assert training
            mean, var = z.mean(0), z.var(0, unbiased=False)
            h = torch.relu((z - mean) / torch.sqrt(var + self.eps) * p[f"g{l}"] + p[f"be{l}"])
        raw = torch.tanh(h @ p["W5"].T + p["b5"])
        if self.att:
            raw = raw * torch.sigmoid(torch.relu(xn @ p["Wa0"].T + p["ba0"]) @ p["Wa1"].T + p["ba1"])
        eb, cb = bounds(self.F, training, self.e, self.dtype)
        pert = torch.nan_to_num(torch.clamp(raw * eb.view(1, -1), -cb.view(1, -1), cb.view(1, -1)), nan=0.0)
        return x + pert, dict(l2_norm=torch.norm(pert, p=2, dim=1).mean(), intensity_loss=pert[:, 3].abs().mean(),
                              bias_loss=pert.mean(dim=0).abs().mean(), imbalance_loss=pert.std(dim=0).std())


def test_fp16_rows_oracle_is_the_oracle_without_rounding():
    """The local subclass restates forward: with the rounding disabled it must give the oracle's own result."""
    case = (M.A16_SHAPES[0][0], M.A16_SHAPES[0][1], 65, True)
    inp = M.standalone_inputs(case)
    plain = type("_PlainRows", (_Fp16RowsOracle,), dict(row_dtype=None))
    a = M.run_oracle_standalone(case, inp, cls=plain, backward=False)
    b = M.run_oracle_standalone(case, inp, backward=False)
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["lvec"], b["lvec"])


@pytest.mark.parametrize("n", M.A16_TAILS)
@pytest.mark.parametrize("shape", M.A16_SHAPES, ids=lambda s: "-".join(map(str, s[0])))
def test_act16_tail_inputs_well_conditioned(shape, n):
    case = (shape[0], shape[1], n, True)
    inp = M.standalone_inputs(case)
    ref = M.run_oracle_standalone(case, inp, backward=False)
    got = M.run_oracle_standalone(case, inp, cls=_Fp16RowsOracle, backward=False)
    assert not np.array_equal(got["out"], ref["out"])        # the rounding is in effect
    ep, el = M.a16_errors(got, ref, inp["x"].astype(np.float64))
    assert ep <= 0.5 * M.A16_TOL and el <= 0.5 * M.A16_TOL, (ep, el)
