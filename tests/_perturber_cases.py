"""Case table of the perturber option matrix (csrc/perturber.hip): seeded inputs, one runner for the HIP
path and one for the CPU oracle, and one comparer with the bounds tests/test_gpu_perturber.py already uses.

Shared by tests/test_gpu_perturber_matrix.py (HIP against the float64 oracle) and
tests/test_perturber_matrix_inputs.py (float32 oracle against the float64 oracle at half the bounds: the
chosen inputs must not be so ill-conditioned that the reference arithmetic itself leaves the bound).
A plain helper module, not a conftest."""
import zlib

import numpy as np
import torch

from oracle.perturber import OraclePerturber, bounds, perturb_voxels

# ---------------------------------------------------------------- bounds (tests/test_gpu_perturber.py)
TOL = 1e-4            # forward / perturbed voxels: atol
LOSS_RTOL = 1e-4      # the four loss terms
LOSS_ATOL = 1e-6
STAT_RTOL = 1e-4      # running mean / var
STAT_ATOL = 1e-5
GRAD_TOL = 2e-3       # every parameter gradient, of that gradient's max-abs
A16_TOL = 5e-3        # 16-bit rows: rel(out - x) and the loss terms against fp32 rows

LOSS_KEYS = ("l2_norm", "intensity_loss", "bias_loss", "imbalance_loss")
CL = np.array([1e-3, -2e-3, 3e-3, 1e-3], np.float32)    # upstream gradient of the loss vector

# 36 parameter slots in rpc_perturber order (include/rpc_hip.h); None = running stats
NAMES = []
for _l in range(5):
    NAMES += [f"W{_l}", f"b{_l}", f"g{_l}", f"be{_l}", None, None]
NAMES += ["W5", "b5", "Wa0", "ba0", "Wa1", "ba1"]
ATT_SLOTS = (32, 33, 34, 35)
# bias of a Linear feeding a train-mode BatchNorm: exact gradient 0, cancellation noise on both sides
NOISE = {f"b{l}" for l in range(5)}

# ---------------------------------------------------------------- the matrix
# one entry per kernel family: VALU 8-channel layers + MFMA; all MFMA (16-bit-capable); the metric's
# widths, F = 4 and 5; wide VALU with global-memory weights and the chunked k_wgrad
WIDTHS = [((8, 16, 32), 4), ((16, 32, 64), 5), ((64, 128, 64), 4), ((64, 128, 64), 5), ((64, 128, 256), 4)]
# below one 64-point group, at and next to a group edge and a 256-thread block edge, several blocks
SIZES = [2, 5, 63, 64, 65, 255, 256, 257, 1000]
EVAL_SIZES = [2, 65, 257]
# one point group past a full sweep of the 256 x 8-wave MFMA grid
LARGE = ((64, 128, 64), 4, 131072 + 65)
A16_SHAPES = [((64, 128, 64), 4), ((16, 32, 64), 5)]
A16_TAILS = [65, 257]
PLUGIN_TAIL = ((12, 24, 40), 4, 65)
# (V, slots, F, vfe_features, training)
FUSED = [(1, 5, 4, 4, True), (13, 5, 4, 4, True), (64, 1, 4, 4, True), (7, 10, 5, 5, True), (7, 10, 5, 4, True),
         (3, 70, 4, 3, True), (300, 5, 4, 4, False), (300, 10, 5, 4, False)]

STANDALONE = [(h, F, n, att) for h, F in WIDTHS for n in SIZES for att in (True, False)]
EVAL = [(h, F, n, att) for h, F in WIDTHS for n in EVAL_SIZES for att in (True, False)]


def sid(c):
    """pytest id of a (hidden, F, N, att) case."""
    h, F, n, att = c
    return f"{'-'.join(map(str, h))}_F{F}_N{n}_{'att' if att else 'noatt'}"


def fid(c):
    V, s, F, vf, tr = c
    return f"V{V}_s{s}_F{F}_vf{vf}_{'train' if tr else 'eval'}"


# seeds: a stable hash of the case; a case whose draw fails the CPU guard gets another seed here
SEEDS = {
    # the hashed seed (and any lower number) left the float32 oracle outside half a bound:
    ("standalone", (64, 128, 64), 5, 2, False): 1,            # loss terms 6.9e-5 off
    ("standalone", (64, 128, 256), 4, 2, False): 2,           # dW0 1.3e-3 of its max-abs; seed 1: a loss term
    ("standalone", (64, 128, 256), 4, 64, False): 1,          # a renumbered evaluation's gradients
    ("standalone", (64, 128, 256), 4, 1000, False): 2,        # dW2 / dW0 (ReLU decisions differ)
    ("standalone", (64, 128, 64), 4, 131072 + 65, True): 2,   # dW0 1.4e-3 of its max-abs
}


def seed_of(*key):
    key = tuple(key)
    return SEEDS.get(key, zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


# ---------------------------------------------------------------- seeded inputs
def make_weights(seed, F, hidden, att=True, running=False):
    """W0..W5, b0..b5 ~ N(0, 1/sqrt(fan_in)); g in [0.5, 1.5], be in [-0.2, 0.2]; Wa0..ba1 when att.
    running: also rm0..rm4 ~ N(0, 0.3), rv0..rv4 in [0.5, 1.5] (eval-mode cases without a train step)."""
    rng = np.random.default_rng(seed)
    widths = [F, hidden[0], hidden[1], hidden[2], hidden[1], hidden[0], F]
    w = {}
    for l in range(6):
        s = 1.0 / np.sqrt(widths[l])
        w[f"W{l}"] = (rng.standard_normal((widths[l + 1], widths[l])) * s).astype(np.float32)
        w[f"b{l}"] = (rng.standard_normal(widths[l + 1]) * s).astype(np.float32)
    for l in range(5):
        w[f"g{l}"] = rng.uniform(0.5, 1.5, widths[l + 1]).astype(np.float32)
        w[f"be{l}"] = rng.uniform(-0.2, 0.2, widths[l + 1]).astype(np.float32)
    A = max(F // 2, 1)
    wa = {"Wa0": (rng.standard_normal((A, F)) / np.sqrt(F)).astype(np.float32),
          "ba0": (rng.standard_normal(A) / np.sqrt(F)).astype(np.float32),
          "Wa1": (rng.standard_normal((1, A)) / np.sqrt(A)).astype(np.float32),
          "ba1": (rng.standard_normal(1) / np.sqrt(A)).astype(np.float32)}
    if att:
        w.update(wa)
    if running:
        for l in range(5):
            w[f"rm{l}"] = (rng.standard_normal(widths[l + 1]) * 0.3).astype(np.float32)
            w[f"rv{l}"] = rng.uniform(0.5, 1.5, widths[l + 1]).astype(np.float32)
    return w


def make_points(seed, N, F):
    """(x, y, z, intensity) scaled [20, 20, 1, 0.3] like the existing tests; F = 5 adds a time lag in [0, 0.5)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, 4)) * np.array([20.0, 20.0, 1.0, 0.3])
    if F == 5:
        x = np.concatenate([x, rng.uniform(0.0, 0.5, (N, 1))], axis=1)
    return x.astype(np.float32)


def make_upstream(seed, shape):
    return (np.random.default_rng(seed).standard_normal(shape) * 1e-3).astype(np.float32)


def make_voxels(seed, V, slots, F):
    """num_points >= 1 everywhere (the first voxel full), slots past num_points zero, and one real slot whose
    features sum to exactly zero (the reference's mask drops it, adversarial_voxelnet.py:89)."""
    rng = np.random.default_rng(seed)
    pool = make_points(seed + 1, max(4 * V, 64), F)
    npts = rng.integers(1, slots + 1, V).astype(np.int32)
    npts[0] = slots
    vox = np.zeros((V, slots, F), np.float32)
    for v in range(V):
        vox[v, :npts[v]] = pool[rng.integers(0, len(pool), npts[v])]
    vox[min(5, V - 1), 0] = [1.0, -1.0] + [0.0] * (F - 2)
    return vox, npts


def plugin_perturber(seed, hidden, att):
    """The plugin module (initialised on the host, as test_plugin_arbitrary_widths_match_oracle does) with
    non-trivial BatchNorm affine parameters, and its weights in the fixture naming."""
    from robustpointclouds_amd.plugin.models.adversarial.voxel_perturber import VoxelPerturber
    torch.manual_seed(seed)
    vp = VoxelPerturber(hidden_channels=list(hidden), use_spatial_attention=att).train()
    lin = [m for m in vp.model if isinstance(m, torch.nn.Linear)]
    bns = [m for m in vp.model if isinstance(m, torch.nn.BatchNorm1d)]
    w = {}
    for l, m in enumerate(lin):
        w[f"W{l}"], w[f"b{l}"] = m.weight.detach().numpy().copy(), m.bias.detach().numpy().copy()
    for l, m in enumerate(bns):
        with torch.no_grad():
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.2, 0.2)
        w[f"g{l}"], w[f"be{l}"] = m.weight.detach().numpy().copy(), m.bias.detach().numpy().copy()
    if att:
        for l, m in enumerate(m for m in vp.attention if isinstance(m, torch.nn.Linear)):
            w[f"Wa{l}"], w[f"ba{l}"] = m.weight.detach().numpy().copy(), m.bias.detach().numpy().copy()
    return vp, w


def plugin_grads(vp):
    lin = [m for m in vp.model if isinstance(m, torch.nn.Linear)]
    bns = [m for m in vp.model if isinstance(m, torch.nn.BatchNorm1d)]
    got = {}
    for l, m in enumerate(lin):
        got[f"W{l}"], got[f"b{l}"] = m.weight.grad, m.bias.grad
    for l, m in enumerate(bns):
        got[f"g{l}"], got[f"be{l}"] = m.weight.grad, m.bias.grad
    if vp.attention is not None:
        for l, m in enumerate(m for m in vp.attention if isinstance(m, torch.nn.Linear)):
            got[f"Wa{l}"], got[f"ba{l}"] = m.weight.grad, m.bias.grad
    return {k: g.detach().cpu().numpy() for k, g in got.items()}


# ---------------------------------------------------------------- inputs of a case
def standalone_inputs(case, eval_half=False):
    hidden, F, N, att = case
    s = seed_of("standalone", *case)
    d = dict(w=make_weights(s, F, hidden, att), x=make_points(s + 1, N, F), G=make_upstream(s + 2, (N, F)))
    if eval_half:
        d["x_eval"] = make_points(s + 3, N, F)
    return d


def fused_inputs(case):
    V, slots, F, vf, training = case
    s = seed_of("fused", *case)
    hidden = (64, 128, 64) if F == 5 else (8, 16, 32)
    vox, npts = make_voxels(s + 1, V, slots, F)
    return dict(hidden=hidden, w=make_weights(s, F, hidden, True, running=not training), vox=vox, npts=npts,
                G=make_upstream(s + 2, (V, vf)))


# ---------------------------------------------------------------- HIP runner
def hip_params(w, F, hidden, dev, att=True, grad=True):
    """36 tensors in rpc_perturber order; running stats from w's rm / rv when present, else (0, 1)."""
    widths = [F, hidden[0], hidden[1], hidden[2], hidden[1], hidden[0]]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev).contiguous()
    ps = []
    for l in range(5):
        rm = t(w[f"rm{l}"]) if f"rm{l}" in w else torch.zeros(widths[l + 1], device=dev)
        rv = t(w[f"rv{l}"]) if f"rv{l}" in w else torch.ones(widths[l + 1], device=dev)
        ps += [t(w[f"W{l}"]), t(w[f"b{l}"]), t(w[f"g{l}"]), t(w[f"be{l}"]), rm, rv]
    ps += [t(w["W5"]), t(w["b5"])]
    ps += [t(w[k]) for k in ("Wa0", "ba0", "Wa1", "ba1")] if att else [None] * 4
    if grad:
        for k, p in enumerate(ps):
            if p is not None and NAMES[k] is not None:
                p.requires_grad_(True)
    return ps


def _np(t):
    return t.detach().cpu().numpy()


def _stats(ps):
    return [_np(ps[6 * l + 4]) for l in range(5)], [_np(ps[6 * l + 5]) for l in range(5)]


def run_hip_standalone(case, inp, split=False, act16=0, backward=True, double_sums=True):
    """One train step of PerturberFn through make_cfg (+ an eval forward with the updated running stats when
    inp has x_eval). grad_slots is what the backward returned for the 36 parameter slots. double_sums=False is
    the bf16 trainer's setting (float batch sums, rpc_perturber_cfg.double_sums)."""
    from robustpointclouds_amd import perturb as P
    hidden, F, N, att = case
    dev = torch.device("cuda")
    ps = hip_params(inp["w"], F, hidden, dev, att)
    cfg = P.make_cfg(F, list(hidden), att, True, 0.2, wgrad_split_bf16=split, act16=act16, double_sums=double_sums)
    out, lvec, flags = P.PerturberFn.apply(torch.from_numpy(inp["x"]).to(dev), cfg, *ps)
    res = dict(out=_np(out), lvec=_np(lvec), flags=_np(flags))
    if backward:
        # the Function's backward called directly, not autograd's .grad: with attention off the four attention
        # parameters are absent, and only the returned tuple shows that their slots come back as None
        ret = P.PerturberFn.backward(out.grad_fn, torch.from_numpy(inp["G"]).to(dev), torch.from_numpy(CL).to(dev),
                                     None)
        slots = ret[2:]
        assert len(slots) == len(NAMES)
        res["grad_slots"] = slots
        res["grads"] = {n: _np(slots[k]) for k, n in enumerate(NAMES) if n is not None and slots[k] is not None}
    res["rm"], res["rv"] = _stats(ps)
    if "x_eval" in inp:
        cfg_e = P.make_cfg(F, list(hidden), att, False, 0.2, double_sums=double_sums)
        with torch.no_grad():
            oute, lve, _ = P.PerturberFn.apply(torch.from_numpy(inp["x_eval"]).to(dev), cfg_e, *ps)
        res["out_eval"], res["l2_eval"] = _np(oute), float(lve[0])
    return res


def run_hip_fused(case, inp, double_sums=True):
    from robustpointclouds_amd import perturb as P
    V, slots, F, vf, training = case
    dev = torch.device("cuda")
    hidden = inp["hidden"]
    ps = hip_params(inp["w"], F, hidden, dev, True, grad=training)
    cfg = P.make_cfg(F, list(hidden), True, training, 0.2, vfe_features=vf, double_sums=double_sums)
    vt, nt = torch.from_numpy(inp["vox"]).to(dev), torch.from_numpy(inp["npts"]).to(dev)
    with torch.set_grad_enabled(training):
        vfe, lvec, pert, flags = P.PerturbVoxelsFn.apply(vt, nt, cfg, *ps)
    res = dict(vfe=_np(vfe), lvec=_np(lvec), pert=_np(pert), flags=_np(flags), nvalid=int(flags[4].item()))
    if training:
        ((vfe * torch.from_numpy(inp["G"]).to(dev)).sum() + (lvec * torch.from_numpy(CL).to(dev)).sum()).backward()
        res["grads"] = {n: _np(ps[k].grad) for k, n in enumerate(NAMES) if n is not None}
        res["rm"], res["rv"] = _stats(ps)
    return res


# ---------------------------------------------------------------- oracle runner
def _oracle(w, F, hidden, dtype, att, cls=OraclePerturber):
    op = cls(w, F, list(hidden), dtype=dtype, use_attention=att)
    for l in range(5):
        if f"rm{l}" in w:
            op.rm[l] = torch.tensor(w[f"rm{l}"], dtype=dtype)
            op.rv[l] = torch.tensor(w[f"rv{l}"], dtype=dtype)
    return op


def _lvec(ld):
    return torch.stack([ld[k] for k in LOSS_KEYS])


def _finish(op, res, head, lv, G, dtype):
    (head * torch.from_numpy(G).to(dtype)).sum().add((lv * torch.from_numpy(CL).to(dtype)).sum()).backward()
    res["grads"] = {k[1:]: g.numpy() for k, g in op.grads().items()}
    res["rm"], res["rv"] = [t.numpy() for t in op.rm], [t.numpy() for t in op.rv]


def renumber_channels(w, F, hidden, seed):
    """The same network with its hidden channels renumbered: every result is mathematically unchanged, but each
    matrix product and channel sum runs in another order, so a float32 evaluation rounds differently.
    Returns (weights, perms) with perms[l] the new order of layer l's input channels."""
    rng = np.random.default_rng(seed)
    widths = [F, hidden[0], hidden[1], hidden[2], hidden[1], hidden[0], F]
    perms = [np.arange(F)] + [rng.permutation(c) for c in widths[1:6]] + [np.arange(F)]
    w2 = dict(w)
    for l in range(6):
        w2[f"W{l}"] = np.ascontiguousarray(w[f"W{l}"][perms[l + 1]][:, perms[l]])
        for k in (f"b{l}", f"g{l}", f"be{l}", f"rm{l}", f"rv{l}"):
            if k in w:
                w2[k] = np.ascontiguousarray(w[k][perms[l + 1]])
    return w2, perms


# layer whose output channels index a per-channel parameter (attention parameters have no hidden channels)
_CHANNEL_LAYER = {f"{k}{l}": l for l in range(6) for k in ("b", "g", "be") if k == "b" or l < 5}


def _original_numbering(res, perms):
    for name, g in res.get("grads", {}).items():
        o = np.empty_like(g)
        if name in {f"W{l}" for l in range(6)}:
            l = int(name[1:])
            o[np.ix_(perms[l + 1], perms[l])] = g
        elif name in _CHANNEL_LAYER:
            o[perms[_CHANNEL_LAYER[name] + 1]] = g
        else:
            continue
        res["grads"][name] = o
    for k in ("rm", "rv"):
        for l, t in enumerate(res.get(k, [])):
            o = np.empty_like(t)
            o[perms[l + 1]] = t
            res[k][l] = o
    return res


def run_oracle_standalone(case, inp, dtype=torch.float64, cls=OraclePerturber, backward=True, renumber=0):
    """renumber != 0: evaluate with the hidden channels renumbered (seeded by it), results mapped back."""
    hidden, F, N, att = case
    if renumber:
        w2, perms = renumber_channels(inp["w"], F, hidden, renumber)
        return _original_numbering(run_oracle_standalone(case, dict(inp, w=w2), dtype, cls, backward), perms)
    op = _oracle(inp["w"], F, hidden, dtype, att, cls)
    out, ld = op.forward(torch.from_numpy(inp["x"]))
    lv = _lvec(ld)
    res = dict(out=out.detach().numpy(), lvec=lv.detach().numpy())
    if backward:
        _finish(op, res, out, lv, inp["G"], dtype)
    if "x_eval" in inp:
        with torch.no_grad():
            oute, lde = op.forward(torch.from_numpy(inp["x_eval"]), training=False)
        res["out_eval"], res["l2_eval"] = oute.numpy(), float(lde["l2_norm"])
    return res


def run_oracle_fused(case, inp, dtype=torch.float64):
    V, slots, F, vf, training = case
    op = _oracle(inp["w"], F, inp["hidden"], dtype, True)
    with torch.set_grad_enabled(training):
        vfe, pert, ld = perturb_voxels(op, inp["vox"], inp["npts"], vfe_features=vf, training=training)
    lv = _lvec(ld)
    res = dict(vfe=vfe.detach().numpy(), lvec=lv.detach().numpy(), pert=pert.detach().numpy(),
               nvalid=int((inp["vox"].reshape(-1, F).sum(1) != 0).sum()))
    if training:
        _finish(op, res, vfe, lv, inp["G"], dtype)
    return res


# ---------------------------------------------------------------- comparer
def compare(got, ref, frac=1.0, imb_atol=0.0, grad_extra=None):
    """Every quantity ref holds against got, within frac of the project's bounds (module head). imb_atol /
    grad_extra: what float_sums_allowance() adds for the imbalance loss (absolute) and per gradient (of its
    max-abs) in the two float-sums cases it is derived for."""
    for k in ("out", "vfe", "pert", "out_eval"):
        if k in ref:
            np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=frac * TOL, err_msg=k)
    np.testing.assert_allclose(got["lvec"][:3], ref["lvec"][:3], rtol=frac * LOSS_RTOL, atol=frac * LOSS_ATOL,
                               err_msg="lvec")
    np.testing.assert_allclose(got["lvec"][3], ref["lvec"][3], rtol=frac * LOSS_RTOL, atol=frac * LOSS_ATOL + imb_atol,
                               err_msg="imbalance_loss")
    if "l2_eval" in ref:
        np.testing.assert_allclose(got["l2_eval"], ref["l2_eval"], rtol=frac * LOSS_RTOL, err_msg="l2_eval")
    if "nvalid" in ref:
        assert got["nvalid"] == ref["nvalid"]
    for k in ("rm", "rv"):
        for l, r in enumerate(ref.get(k, [])):
            np.testing.assert_allclose(got[k][l], r, rtol=frac * STAT_RTOL, atol=frac * STAT_ATOL, err_msg=f"{k}{l}")
    for name, r in ref.get("grads", {}).items():
        if name in NOISE:
            continue
        g = got["grads"][name]
        assert g.shape == r.shape, name
        np.testing.assert_allclose(g, r, rtol=0, atol=(frac * GRAD_TOL + (grad_extra or {}).get(name, 0.0)) * max(np.abs(r).max(), 1e-6),
                                   err_msg="d" + name)


# The two cases of the matrix where float batch sums (rpc_perturber_cfg.double_sums = 0, the bf16 trainer's setting)
# cannot meet the parity bounds, each with two points:
FLOAT_SUMS_CASES = {
    ((64, 128, 64), 4, 2, False): "imbalance",   # both points' intensity perturbation sits on the clamp: true std 0
    ((64, 128, 64), 4, 2, True): "gradients",    # the channels that carry the gradient have |mean| >> std
}
U = 2.0 ** -24    # unit roundoff of float32


class _ShiftedVarianceOracle(OraclePerturber):
    """OraclePerturber's train-mode forward with the batch variance of the MFMA hidden layers (1..4) moved by
    sign * (n + 2) U E[z^2], the most a one-pass float variance can be off (float_sums_allowance)."""
    sign = 1.0

    def forward(self, x, training=True):
        p = self.p
        x = torch.as_tensor(x).to(self.dtype)
        xn = torch.clamp(x / (torch.std(x, dim=0, keepdim=True) + 1e-6), -10.0, 10.0)
        h, n = xn, x.shape[0]
        for l in range(5):
            z = h @ p[f"W{l}"].T + p[f"b{l}"]
            mean, var = z.mean(0), z.var(0, unbiased=False)
            if l >= 1:
                var = (var + (self.sign * (n + 2) * U * (z * z).mean(0)).detach()).clamp_min(0.0)
            h = torch.relu((z - mean) / torch.sqrt(var + self.eps) * p[f"g{l}"] + p[f"be{l}"])
        raw = torch.tanh(h @ p["W5"].T + p["b5"])
        if self.att:
            raw = raw * torch.sigmoid(torch.relu(xn @ p["Wa0"].T + p["ba0"]) @ p["Wa1"].T + p["ba1"])
        eb, cb = bounds(self.F, training, self.e, self.dtype)
        pert = torch.clamp(raw * eb.view(1, -1), -cb.view(1, -1), cb.view(1, -1))
        return x + pert, dict(l2_norm=torch.norm(pert, p=2, dim=1).mean(), intensity_loss=pert[:, 3].abs().mean(),
                              bias_loss=pert.mean(dim=0).abs().mean(), imbalance_loss=pert.std(dim=0).std())


def float_sums_allowance(case, inp, ref):
    """(imb_atol, grad_extra) for a FLOAT_SUMS_CASES case, from the float64 oracle (ref: its result) and float32's
    roundoff alone; grad_extra maps a gradient's name to a fraction of its max-abs.

    Float sums of n float squares carry at most (n + 1) U of relative error (n roundings of the squares, n - 1 of
    the additions, one of n mean^2), so a one-pass variance sum z^2 / n - mean^2 is off by at most (n + 2) U E[z^2].
    imbalance: a feature whose n perturbations are all p keeps a std of at most |p| sqrt((n + 2) U n / (n - 1))
    where it is 0, and the std over features moves by no more than one feature's std does.
    gradients: the float64 oracle evaluated with every hidden variance moved by that much, upwards and downwards:
    how far each gradient moves (the larger of the two) is what the float sums may add to the parity bound."""
    hidden, F, n, att = case
    if FLOAT_SUMS_CASES[case] == "imbalance":
        pmax = float(bounds(F, True, 0.2, torch.float64)[1].max())
        return pmax * float(np.sqrt((n + 2) * U * n / (n - 1))), {}
    extra = {}
    for sign in (1.0, -1.0):
        got = run_oracle_standalone(case, inp, cls=type("_Shifted", (_ShiftedVarianceOracle,), dict(sign=sign)))
        for name, r in ref["grads"].items():
            e = float(np.abs(got["grads"][name] - r).max() / max(np.abs(r).max(), 1e-6))
            extra[name] = max(extra.get(name, 0.0), e)
    return 0.0, extra


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))


def a16_errors(got, ref, x):
    """rel(out - x) and the worst relative loss-term error of a 16-bit-rows run against the fp32-rows run."""
    ep = rel(got["out"].astype(np.float64) - x, ref["out"].astype(np.float64) - x)
    el = max(abs(float(a) - float(b)) / max(abs(float(b)), 1e-12) for a, b in zip(got["lvec"], ref["lvec"]))
    return ep, el
