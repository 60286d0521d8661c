"""TEST INFRASTRUCTURE ONLY: a float64 eval-mode SparseEncoder (BatchNorm with the running statistics) on the CPU.

Restates upstream mmdet3d `SparseEncoder` under `model.eval()`: per layer the sparse convolution
(SubMConv3d / SparseConv3d semantics of oracle/sparse_encoder.py, whose rulebook functions are imported),
`(z - running_mean) / sqrt(running_var + eps) * gamma + beta`, the SparseBasicBlock identity where the
layer closes a block, ReLU, and at the end `.dense()` viewed as [B, C*D, H, W]. Nothing depends on the
other rows of the batch and no statistic is updated. Weights and statistics are copied from the module
(or given explicitly); no code is shared with the package under test.

`h16_from` / `fp16` emulate the 16-bit engine's operand formats as OracleSparseEncoder(bf16_from=,
fwd_fp16=) does: from that layer on, the gathered input rows and the weights are rounded to bf16 (fp16)
before the products; everything else stays float64 — the error an engine with those operands cannot avoid.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import voxelize as ov
from oracle.sparse_encoder import spconv_pairs, subm_pairs
from robustpointclouds_amd.synthetic import KITTI_PC_RANGE, KITTI_VOXEL_SIZE, kitti_frame

SPARSE_SHAPE = [41, 1600, 1408]
BASIC = dict(output_channels=128, encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
             encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, [0, 1, 1]), (1, 1)), block_type="basicblock")


def frames_input(seeds, stride=4, extra_feature=False):
    """Voxel features (the VFE mean) and coordinates of decimated synthetic KITTI frames, one per seed.
    extra_feature: a fifth input feature (the nuScenes time lag's slot)."""
    frames = [kitti_frame(s)[::stride] for s in seeds]
    vox, coors, npts = ov.voxelize_frames(frames, KITTI_VOXEL_SIZE, KITTI_PC_RANGE, 5, 16000)
    feats = (vox[:, :, :4].sum(1) / npts[:, None]).astype(np.float32)
    if extra_feature:
        feats = np.concatenate([feats, np.random.default_rng(4).uniform(0, 0.5, (len(feats), 1))], 1)
    return feats.astype(np.float32), coors.astype(np.int32)


def randomize_bn(enc, seed=5):
    """Non-trivial affine parameters and running statistics on every BatchNorm of a SparseEncoder."""
    g = torch.Generator().manual_seed(seed)
    u = lambda n, lo, hi: torch.rand(n, generator=g) * (hi - lo) + lo
    with torch.no_grad():
        for _, bn in enc.layers():
            c = bn.num_features
            bn.weight.copy_(u(c, 0.5, 1.5))
            bn.bias.copy_(u(c, -0.2, 0.2))
            bn.running_mean.copy_(u(c, -0.1, 0.1))
            bn.running_var.copy_(u(c, 0.5, 2.0))


def _round(t, fmt):
    if fmt is None:
        return t
    return t.to(torch.float16 if fmt == "fp16" else torch.bfloat16).to(t.dtype)


class EvalSparseRef:
    def __init__(self, enc, h16_from=None, fp16=False, stats=None):
        """enc: a SparseEncoder (its specs, shapes, weights, BatchNorm parameters and running statistics are
        copied); stats (optional): per layer (running_mean, running_var) to use instead of the module's."""
        self.specs = [(sp.kind, tuple(sp.ksize), tuple(sp.stride), tuple(sp.pad), sp.key, sp.lvl_in, sp.lvl_out,
                       sp.co, sp.res) for sp in enc.specs]
        self.shapes = [tuple(s) for s in enc.shapes]
        self.h16_from = h16_from
        self.fmt = None if h16_from is None else ("fp16" if fp16 else "bf16")
        f64 = lambda t: t.detach().cpu().double().clone()
        self.layers = []
        for li, (conv, bn) in enumerate(enc.layers()):
            rm, rv = (bn.running_mean, bn.running_var) if stats is None else stats[li]
            self.layers.append(dict(W=f64(conv.weight), g=f64(bn.weight), b=f64(bn.bias), rm=f64(rm), rv=f64(rv),
                                    eps=float(bn.eps)))

    def forward(self, feats, coors, B):
        x = torch.as_tensor(np.asarray(feats)).double()
        c = np.asarray(coors, np.int64)
        books = {}
        outs = []
        for li, ((kind, ksize, stride, pad, key, lin, lout, co, res), p) in enumerate(zip(self.specs, self.layers)):
            if kind == "subm":
                if key not in books:
                    books[key] = subm_pairs(c, (B,) + self.shapes[lin], ksize)
                pairs, c_out, n_out = books[key], c, x.shape[0]
            else:
                c_out, pairs = spconv_pairs(c, (B,) + self.shapes[lout], ksize, stride, pad)
                n_out = c_out.shape[0]
            fmt = self.fmt if (self.h16_from is not None and li >= self.h16_from) else None
            xg, Wg = _round(x, fmt), _round(p["W"], fmt)
            z = torch.zeros((n_out, co), dtype=torch.float64)
            for k, (ri, ro) in enumerate(pairs):
                if len(ri):
                    z = z.index_add(0, torch.from_numpy(ro), xg[torch.from_numpy(ri)] @ Wg[k])
            pre = (z - p["rm"]) / torch.sqrt(p["rv"] + p["eps"]) * p["g"] + p["b"]
            if res >= 0:
                pre = pre + outs[res]
            x = torch.relu(pre)
            outs.append(x)
            c = c_out
        D, H, W = self.shapes[-1]
        C = x.shape[1]
        dense = torch.zeros((B, D, H, W, C), dtype=torch.float64)
        dense[torch.from_numpy(c[:, 0]), torch.from_numpy(c[:, 1]), torch.from_numpy(c[:, 2]),
              torch.from_numpy(c[:, 3])] = x
        return dense.permute(0, 4, 1, 2, 3).reshape(B, C * D, H, W)
