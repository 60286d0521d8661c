"""SparseEncoder under eval(): BatchNorm with the running statistics, on both engines, against the float64
eval-mode reference of tests/_sparse_eval_ref.py (pinned by tests/test_sparse_eval_ref_cpu.py).

Decimated synthetic KITTI frames (about 3-4k voxels each) at the config's sparse shape; the first 1 / 63 / 64 / 65
voxels of a frame cover the edges of a 64-row tile and strided layers whose output count is far below a tile."""
import functools

import numpy as np
import pytest
import torch

from robustpointclouds_amd import sparse_encoder as SE
from robustpointclouds_amd.sparse_encoder import SparseEncoder
from tests._sparse_eval_ref import BASIC, SPARSE_SHAPE, EvalSparseRef, frames_input, randomize_bn

pytestmark = pytest.mark.gpu

ENCODERS = ["second", "nus"]   # conv_module (SECOND) / basicblock with 5 input features (CenterPoint nuScenes)
INPUTS = ["b2", "b2_empty", "n1", "n63", "n64", "n65"]


@functools.lru_cache(maxsize=None)
def _input(kind, name):
    """(feats, coors, B), read-only."""
    if name == "b2":
        f, c = frames_input([0, 1], extra_feature=kind == "nus")
        return f, c, 2
    f, c = frames_input([0], extra_feature=kind == "nus")
    if name == "b2_empty":     # a batch of two whose second frame has no voxel
        return f, c, 2
    n = int(name[1:])
    return f[:n].copy(), c[:n].copy(), 1


def _encoder(kind, dev="cuda", bf16=False):
    torch.manual_seed(0)
    enc = SparseEncoder(5 if kind == "nus" else 4, SPARSE_SHAPE, **(BASIC if kind == "nus" else {}))
    randomize_bn(enc)
    enc = enc.to(dev)
    enc.bf16 = bf16
    return enc.eval()


@functools.lru_cache(maxsize=None)
def _reference(kind, name, fmt=None):
    """The float64 eval reference (fmt 'fp16' / 'bf16': with the 16-bit engine's operand rounding from layer 1 on)
    of the encoder _encoder(kind) on input `name`; computed once, never modified."""
    f, c, B = _input(kind, name)
    enc = _encoder(kind, "cpu")
    ref = EvalSparseRef(enc, h16_from=None if fmt is None else 1, fp16=fmt == "fp16")
    return ref.forward(f, c, B)


def _run(enc, kind, name):
    f, c, B = _input(kind, name)
    with torch.no_grad():
        out = enc(torch.from_numpy(f).cuda(), torch.from_numpy(c).cuda(), B)
    return out.float().cpu().double()   # (a copy: the dense image is the module's persistent buffer)


def _state(enc):
    return {k: v.detach().cpu().clone() for k, v in enc.state_dict().items()}


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        np.array_equal(a.reshape(-1).numpy().view(np.uint8), b.reshape(-1).numpy().view(np.uint8))


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("kind", ENCODERS)
def test_fp32_engine_matches_eval_reference(kind, name):
    ref = _reference(kind, name)
    out = _run(_encoder(kind), kind, name)
    assert out.shape == ref.shape
    err, scale = float((out - ref).abs().max()), float(ref.abs().max())
    print(f"{kind} {name}: fp32 engine max |out - ref| {err:.3e}, max |ref| {scale:.3e}")
    assert scale > 0
    assert err <= 1e-4 * max(scale, 1.0)     # the fp32 forward bar of tests/test_gpu_sparse_encoder.py


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("kind", ENCODERS)
def test_h16_engine_within_its_operand_rounding(kind, fmt, name, monkeypatch):
    """The bar of tests/test_gpu_sparse_layers.py: the engine's distance from the plain float64 reference against
    the distance of the same reference with the operands rounded where the kernels round them."""
    monkeypatch.setattr(SE, "FWD_FMT", 1 if fmt == "fp16" else 0)
    ref, emu = _reference(kind, name), _reference(kind, name, fmt)
    out = _run(_encoder(kind, bf16=True), kind, name)
    d_eng, d_emu = _rel(out, ref), _rel(emu, ref)
    print(f"{kind} {fmt} {name}: rel L2 from float64: engine {d_eng:.3e}, operand-rounding reference {d_emu:.3e}")
    assert float(ref.norm()) > 0
    assert d_eng <= max(0.05, 1.1 * d_emu)
    assert d_eng < 3e-2                       # test_bf16_perf_mode_close_to_oracle's


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kind", ENCODERS)
def test_eval_forward_leaves_the_statistics_alone(kind, bf16):
    enc = _encoder(kind, bf16=bf16)
    before = _state(enc)
    assert any(k.endswith("num_batches_tracked") for k in before)
    _run(enc, kind, "b2")
    torch.cuda.synchronize()
    after = _state(enc)
    for k in before:
        assert _same_bytes(before[k], after[k]), k
    # (a train-mode forward does move them: the comparison can see it)
    enc.train()
    _run(enc, kind, "n65")
    moved = _state(enc)
    assert not all(_same_bytes(before[k], moved[k]) for k in before if "running_mean" in k)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kind", ENCODERS)
def test_eval_output_does_not_depend_on_the_batch(kind, bf16):
    """Frame a (b) alone gives the dense slice it has in the batch {a, b}: no eval kernel reduces across rows."""
    f, c, _ = _input(kind, "b2")
    enc = _encoder(kind, bf16=bf16)

    def fwd(rows, B, batch0=False):
        cc = c[rows].copy()
        if batch0:
            cc[:, 0] = 0
        with torch.no_grad():
            return enc(torch.from_numpy(f[rows]).cuda(), torch.from_numpy(cc).cuda(), B).float().cpu().clone()

    ia, ib = c[:, 0] == 0, c[:, 0] == 1
    assert ia.sum() > 1000 and ib.sum() > 1000
    both = fwd(np.ones(len(c), bool), 2)
    scale = float(both.abs().max())
    for tag, alone, got in (("a", fwd(ia, 1), both[0:1]), ("b", fwd(ib, 1, batch0=True), both[1:2])):
        diff = float((alone - got).abs().max())
        print(f"{kind} bf16={bf16} frame {tag}: alone vs in the batch max |diff| {diff:.3e} (max |out| {scale:.3e}); "
              f"bit-identical: {torch.equal(alone, got)}")
        assert diff <= 1e-5 * scale
    if kind == "second" and not bf16:   # batch statistics do depend on the batch: the comparison can see it
        enc.train()
        both_t, alone_t = fwd(np.ones(len(c), bool), 2), fwd(ia, 1)
        assert float((alone_t - both_t[0:1]).abs().max()) > 1e-3 * float(both_t.abs().max())


@pytest.mark.parametrize("bf16", [False, True])
def test_backward_through_eval_forward_raises(bf16):
    f, c, B = _input("second", "n65")
    enc = _encoder("second", bf16=bf16)
    x = torch.from_numpy(f).cuda().requires_grad_(True)
    out = enc(x, torch.from_numpy(c).cuda(), B)
    with pytest.raises(RuntimeError, match="eval"):
        out.float().sum().backward()


@pytest.mark.parametrize("kind", ENCODERS)
def test_weight_tiles_follow_the_weights(kind):
    """eval -> train (a step that writes the weights in place, behind autograd's version counters, as the fused
    optimizer does) -> eval: the cached 16-bit tiles are rebuilt."""
    f, c, B = _input(kind, "b2")
    ft, ct = torch.from_numpy(f).cuda(), torch.from_numpy(c).cuda()
    enc = _encoder(kind, bf16=True)
    with torch.no_grad():
        first = enc(ft, ct, B).clone()
        again = enc(ft, ct, B).clone()
    assert torch.equal(first, again)            # (the second forward ran on the cached tiles)
    enc.train()
    out = enc(ft, ct, B)
    out.float().square().mean().backward()
    with torch.no_grad():
        for p in enc.parameters():
            step = 0.05 * p.data.abs().mean() * torch.sign(p.grad)
            p.data.sub_(step)                   # `.data`: p._version does not move
            p.grad = None
    enc.eval()
    with torch.no_grad():
        got = enc(ft, ct, B).clone()
    fresh = _encoder(kind, bf16=True)
    fresh.load_state_dict(enc.state_dict())
    with torch.no_grad():
        want = fresh(ft, ct, B).clone()
    assert not torch.equal(got, first)
    assert torch.equal(got, want)


def test_bn_fold_matches_its_formula():
    from robustpointclouds_amd import _ffi
    lib = _ffi.load()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(2)
    cs = [1, 16, 37, 128, 300]
    rows = [[torch.rand(c, generator=g).to(dev) + 0.5 for _ in range(4)] for c in cs]   # gamma, beta, mean, var
    outs = [(torch.full((4 * c,), float("nan"), device=dev), torch.full((2 * c,), float("nan"), device=dev))
            for c in cs]
    descs = (_ffi.RpcBnFold * len(cs))()
    for i, (c, r, o) in enumerate(zip(cs, rows, outs)):
        descs[i] = _ffi.RpcBnFold(*[t.data_ptr() for t in r], 1e-3, c, o[0].data_ptr(), o[1].data_ptr())
    _ffi.check(lib.rpc_bn_fold_batch(descs, len(cs), _ffi.stream_of(rows[0][0])), "rpc_bn_fold_batch")
    for c, (gamma, beta, mean, var), (bn, fold) in zip(cs, rows, outs):
        invstd = 1.0 / torch.sqrt(var.double() + np.float32(1e-3).astype(np.float64))
        want_bn = torch.cat([gamma.double() * invstd, beta.double(), mean.double(), invstd])
        want_fold = torch.cat([gamma.double() * invstd, beta.double() - mean.double() * gamma.double() * invstd])
        # fp32 arithmetic of a handful of operations on O(1) values: a few ulp
        assert float((bn.double() - want_bn).abs().max()) <= 1e-6 * float(want_bn.abs().max())
        assert float((fold.double() - want_fold).abs().max()) <= 1e-6 * float(want_fold.abs().max())
        assert torch.equal(bn[:c], fold[:c])
