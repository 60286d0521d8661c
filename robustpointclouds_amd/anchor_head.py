"""Anchor3DHead forward + training targets + losses.

Restates upstream mmdet3d v1.x `Anchor3DHead` (dense_heads/anchor3d_head.py),
`AnchorTrainMixin.anchor_target_3d` (dense_heads/train_mixins.py),
`Anchor3DRangeGenerator` (task_modules/anchor/anchor_3d_generator.py), `Max3DIoUAssigner`
= mmdet `MaxIoUAssigner` with `BboxOverlapsNearest3D` (nearest-BEV IoU),
`DeltaXYZWLHRBBoxCoder`, `get_direction_target`, mmdet `FocalLoss` (sigmoid, mmcv kernel
formulas), `SmoothL1Loss`, `CrossEntropyLoss`, configured at
configs/adversarial/adversarial-second_hv_secfpn_8xb6-80e_kitti-3d-3class.py:38-69 and
:86-112 (3-class) / adversarial-second_hv_secfpn_8xb6-80e_kitti-3d-car.py:18-39 (car).

Upstream returns a dict of LISTS (one tensor per feature level, via multi_apply); this is
kept (`loss_by_feat`), because AdversarialVoxelNet.loss only sums Tensor-valued entries
(SURVEY.md finding 3). Target assignment and losses run as HIP kernels (csrc/anchor_head.hip,
`rpc_anchor_head_loss_forward/backward`) batched over the frames with no host
synchronisation; the three 1x1 convs run as ONE GEMM on the dense engine (P1 map) — bf16
(`rpc_dense_conv` / `rpc_dense_wgrad`) in perf mode, fp32 MFMA (`rpc_dense_conv_f32` /
`rpc_dense_wgrad_f32`) in the fp32 parity mode. The CPU restatement the kernels are checked against is oracle/anchor_head.py.
mmdet3d is not installed here: parity for this row is "unpinned" w.r.t. upstream.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as Fn
from torch import nn

from . import _ffi
from .base_model import det3d_gt

P1 = 3          # dense-engine map: 1x1 conv
HEAD_PAD = 128  # GEMM width of the bf16 head image (the engine's output-channel tile)


def limit_period(val, offset=0.5, period=math.pi):
    return val - torch.floor(val / period + offset) * period


class Anchor3DRangeGenerator:
    def __init__(self, ranges, sizes=((1.6, 3.9, 1.56),), scales=(1,), rotations=(0, 1.5707963),
                 custom_values=(), reshape_out=True, size_per_range=True):
        self.ranges = [list(r) for r in ranges]
        self.sizes = [list(s) for s in sizes]
        self.scales = list(scales)
        self.rotations = list(rotations)
        self.custom_values = list(custom_values)
        self.reshape_out = reshape_out
        self.size_per_range = size_per_range
        if size_per_range and len(self.sizes) == 1:
            self.sizes = self.sizes * len(self.ranges)

    @property
    def num_base_anchors(self):
        return len(self.rotations) * int(torch.tensor(self.sizes).reshape(-1, 3).size(0))

    def anchors_single_range(self, feature_size, anchor_range, scale, sizes, rotations, device):
        if len(feature_size) == 2:
            feature_size = [1, feature_size[0], feature_size[1]]
        r = torch.tensor(anchor_range, device=device)
        zc = torch.linspace(r[2], r[5], feature_size[0], device=device)
        yc = torch.linspace(r[1], r[4], feature_size[1], device=device)
        xc = torch.linspace(r[0], r[3], feature_size[2], device=device)
        sizes = torch.tensor(sizes, device=device).reshape(-1, 3) * scale
        rot = torch.tensor(rotations, device=device)
        rets = list(torch.meshgrid(xc, yc, zc, rot, indexing="ij"))
        tile = [1] * 5
        tile[-2] = int(sizes.shape[0])
        for i in range(len(rets)):
            rets[i] = rets[i].unsqueeze(-2).repeat(tile).unsqueeze(-1)
        sizes = sizes.reshape([1, 1, 1, -1, 1, 3])
        ts = list(rets[0].shape)
        ts[3] = 1
        rets.insert(3, sizes.repeat(ts))
        return torch.cat(rets, dim=-1).permute([2, 1, 0, 3, 4, 5])   # [D, H, W, S, R, 7]

    def single_level_grid_anchors(self, featmap_size, scale, device):
        if not self.size_per_range:
            return self.anchors_single_range(featmap_size, self.ranges[0], scale, self.sizes, self.rotations, device)
        mr = [self.anchors_single_range(featmap_size, rg, scale, sz, self.rotations, device)
              for rg, sz in zip(self.ranges, self.sizes)]
        return torch.cat(mr, dim=-3)

    def grid_anchors(self, featmap_sizes, device):
        out = []
        for i, fs in enumerate(featmap_sizes):
            a = self.single_level_grid_anchors(fs, self.scales[i], device)
            if self.reshape_out:
                a = a.reshape(-1, a.size(-1))
            out.append(a)
        return out


class DeltaXYZWLHRBBoxCoder:
    code_size = 7

    @staticmethod
    def encode(src, dst):
        xa, ya, za, wa, la, ha, ra = torch.split(src, 1, dim=-1)
        xg, yg, zg, wg, lg, hg, rg = torch.split(dst, 1, dim=-1)
        za = za + ha / 2
        zg = zg + hg / 2
        diag = torch.sqrt(la ** 2 + wa ** 2)
        return torch.cat([(xg - xa) / diag, (yg - ya) / diag, (zg - za) / ha, torch.log(wg / wa),
                          torch.log(lg / la), torch.log(hg / ha), rg - ra], dim=-1)

    @staticmethod
    def decode(anchors, deltas):
        xa, ya, za, wa, la, ha, ra = torch.split(anchors, 1, dim=-1)
        xt, yt, zt, wt, lt, ht, rt = torch.split(deltas, 1, dim=-1)
        za = za + ha / 2
        diag = torch.sqrt(la ** 2 + wa ** 2)
        xg, yg = xt * diag + xa, yt * diag + ya
        zg = zt * ha + za
        lg, wg, hg = torch.exp(lt) * la, torch.exp(wt) * wa, torch.exp(ht) * ha
        return torch.cat([xg, yg, zg - hg / 2, wg, lg, hg, rt + ra], dim=-1)


def anchor_table(gen: Anchor3DRangeGenerator, H: int, W: int) -> torch.Tensor:
    """The generator's centres / sizes / rotations as the flat fp32 table the head kernels read:
    xc[S][W], yc[S][H], zc[S], sizes[S][3], rotations[R] (torch.linspace on the host, exactly the
    values anchors_single_range meshes)."""
    xs, ys, zs = [], [], []
    for rg in gen.ranges:
        r = torch.tensor(rg, dtype=torch.float32)
        xs.append(torch.linspace(r[0], r[3], W))
        ys.append(torch.linspace(r[1], r[4], H))
        zs.append(torch.linspace(r[2], r[5], 1))
    sizes = torch.tensor(gen.sizes, dtype=torch.float32).reshape(-1, 3) * gen.scales[0]
    rot = torch.tensor(gen.rotations, dtype=torch.float32)
    return torch.cat([torch.cat(xs), torch.cat(ys), torch.cat(zs), sizes.reshape(-1), rot]).contiguous()


class HeadConvFn(torch.autograd.Function):
    """The fused 1x1 head conv (cls | reg | dir weights stacked, no bias) on the bf16 dense engine:
    x [B, C, H, W] bf16 channels_last -> z [B*H*W, HEAD_PAD] bf16 (channels >= N are zero)."""

    @staticmethod
    def forward(ctx, x, weight):
        from .dense_bev import _nhwc
        lib = _ffi.load()
        x = _nhwc(x)
        B, Cin, H, W = x.shape
        N = weight.shape[0]
        if N > HEAD_PAD or Cin % 128:
            raise RuntimeError(f"HIP head conv needs <= {HEAD_PAD} outputs and C_in % 128 == 0 (got {N}, {Cin})")
        dev = x.device
        st = _ffi.stream_of(x)
        # rows N .. HEAD_PAD-1 written as zero by the kernel (co_src = N): no padded fp32 copy
        w32 = weight.detach().reshape(N, Cin).float().contiguous()
        wf = torch.empty((1, HEAD_PAD, Cin), dtype=torch.bfloat16, device=dev)
        wd = torch.empty((1, Cin, HEAD_PAD), dtype=torch.bfloat16, device=dev)
        desc = (_ffi.RpcDenseWprep * 1)(_ffi.RpcDenseWprep(w32.data_ptr(), wf.data_ptr(), wd.data_ptr(), 0, Cin,
                                                           HEAD_PAD, 1, 0, N))
        _ffi.check(lib.rpc_dense_wprep_batch(desc, 1, st), "rpc_dense_wprep_batch(head)")
        z = torch.empty((B * H * W, HEAD_PAD), dtype=torch.bfloat16, device=dev)
        img = _ffi.int_arr((B, H, W))
        _ffi.check(lib.rpc_dense_conv(P1, _ffi.ptr(x), Cin, Cin, _ffi.ptr(wf), HEAD_PAD, _ffi.ptr(z), HEAD_PAD, 0, 0,
                                      None, img, img, img, st), "rpc_dense_conv(head)")
        ctx.save_for_backward(x, wd)
        ctx.N, ctx.wshape = N, tuple(weight.shape)
        return z

    @staticmethod
    def backward(ctx, dz):
        from .dense_bev import _image
        lib = _ffi.load()
        x, wd = ctx.saved_tensors
        B, Cin, H, W = x.shape
        dev = x.device
        dz = dz.to(torch.bfloat16).contiguous()
        st = _ffi.stream_of(dz)
        img = _ffi.int_arr((B, H, W))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _image(B, Cin, H, W, dev)
            _ffi.check(lib.rpc_dense_conv(P1, _ffi.ptr(dz), HEAD_PAD, HEAD_PAD, _ffi.ptr(wd), Cin, _ffi.ptr(dx), Cin,
                                          0, 0, None, img, img, img, st), "rpc_dense_conv(head dgrad)")
        dw = None
        if ctx.needs_input_grad[1]:
            dwp = torch.empty((HEAD_PAD, Cin, 1, 1), dtype=torch.float32, device=dev)
            wsz = lib.rpc_dense_wgrad_workspace_size(P1, img, Cin, HEAD_PAD)
            ws = _ffi.workspace(wsz, dev)
            _ffi.check(lib.rpc_dense_wgrad(P1, 0, _ffi.ptr(x), Cin, Cin, _ffi.ptr(dz), HEAD_PAD, HEAD_PAD, img, img,
                                           img, _ffi.ptr(dwp), _ffi.ptr(ws), wsz, st), "rpc_dense_wgrad(head)")
            dw = dwp[:ctx.N].reshape(ctx.wshape)
        return dx, dw


def head_pad_f32(N: int) -> int:
    """GEMM width of the fp32 head image: N rounded up to the fp32 engine's 64-channel tile."""
    return (N + 63) // 64 * 64


class HeadConvF32Fn(torch.autograd.Function):
    """The fused 1x1 head conv (no bias) on the fp32 dense engine (parity mode):
    x [B, C, H, W] fp32 -> z [B*H*W, NP] fp32, NP = head_pad_f32(N) (channels >= N are zero)."""

    @staticmethod
    def forward(ctx, x, weight):
        from .dense_bev import _nhwc
        lib = _ffi.load()
        if not x.is_cuda:
            raise RuntimeError("Anchor3DHead runs on the HIP kernels only (no CPU path)")
        x = _nhwc(x, torch.float32)
        B, Cin, H, W = x.shape
        N = weight.shape[0]
        NP = head_pad_f32(N)
        if Cin % 64:
            raise RuntimeError(f"fp32 HIP head conv needs C_in % 64 == 0 (got {Cin})")
        dev = x.device
        st = _ffi.stream_of(x)
        wp = Fn.pad(weight.detach().reshape(N, Cin).float(), (0, 0, 0, NP - N)).contiguous()
        wf = torch.empty((1, NP, Cin), dtype=torch.float32, device=dev)
        wd = torch.empty((1, Cin, NP), dtype=torch.float32, device=dev)
        desc = (_ffi.RpcDenseWprep * 1)()
        desc[0] = _ffi.RpcDenseWprep(wp.data_ptr(), wf.data_ptr(), wd.data_ptr(), 0, Cin, NP, 1, 0)
        _ffi.check(lib.rpc_dense_wprep_batch_f32(desc, 1, st), "rpc_dense_wprep_batch_f32(head)")
        z = torch.empty((B * H * W, NP), dtype=torch.float32, device=dev)
        img = _ffi.int_arr((B, H, W))
        _ffi.check(lib.rpc_dense_conv_f32(P1, _ffi.ptr(x), Cin, Cin, _ffi.ptr(wf), NP, _ffi.ptr(z), NP, 0, 0, None,
                                          img, img, img, st), "rpc_dense_conv_f32(head)")
        ctx.save_for_backward(x, wd, wp)
        ctx.N, ctx.NP, ctx.wshape = N, NP, tuple(weight.shape)
        return z

    @staticmethod
    def backward(ctx, dz):
        from .dense_bev import _image
        lib = _ffi.load()
        x, wd, _ = ctx.saved_tensors
        B, Cin, H, W = x.shape
        NP = ctx.NP
        dev = x.device
        dz = dz.float().contiguous()
        st = _ffi.stream_of(dz)
        img = _ffi.int_arr((B, H, W))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _image(B, Cin, H, W, dev, torch.float32)
            _ffi.check(lib.rpc_dense_conv_f32(P1, _ffi.ptr(dz), NP, NP, _ffi.ptr(wd), Cin, _ffi.ptr(dx), Cin, 0, 0,
                                              None, img, img, img, st), "rpc_dense_conv_f32(head dgrad)")
        dw = None
        if ctx.needs_input_grad[1]:
            dwp = torch.empty((NP, Cin, 1, 1), dtype=torch.float32, device=dev)
            wsz = lib.rpc_dense_wgrad_workspace_size_f32(P1, img, Cin, NP)
            ws = _ffi.workspace(wsz, dev)
            _ffi.check(lib.rpc_dense_wgrad_f32(P1, 0, _ffi.ptr(x), Cin, Cin, _ffi.ptr(dz), NP, NP, img, img, img,
                                               _ffi.ptr(dwp), _ffi.ptr(ws), wsz, st), "rpc_dense_wgrad_f32(head)")
            dw = dwp[:ctx.N].reshape(ctx.wshape)
        return dx, dw


class HeadLossFn(torch.autograd.Function):
    """(z, bias) -> [loss_cls, loss_bbox, loss_dir] through rpc_anchor_head_loss_forward/backward."""

    @staticmethod
    def forward(ctx, z, bias, head, layout, gt_boxes, gt_labels):
        lib = _ffi.load()
        if not z.is_cuda:
            raise RuntimeError("Anchor3DHead loss runs on the HIP kernels only (no CPU path)")
        cfg, tab = head._kernel_cfg(layout, z.device)
        M = int(gt_boxes.shape[1])
        gb = gt_boxes.float().contiguous()
        gl = gt_labels.to(torch.int64).contiguous()
        A = cfg.S * cfg.R
        asg = torch.empty((cfg.B, cfg.H * cfg.W * A), dtype=torch.int32, device=z.device)
        out = torch.empty(4, dtype=torch.float32, device=z.device)
        wsz = lib.rpc_anchor_head_workspace_size(C.byref(cfg), M)
        ws = _ffi.workspace(wsz, z.device)
        bias = bias.detach().float().contiguous()
        _ffi.check(lib.rpc_anchor_head_loss_forward(C.byref(cfg), _ffi.ptr(tab), _ffi.ptr(gb), _ffi.ptr(gl), M,
                                                    _ffi.ptr(z), _ffi.ptr(bias), _ffi.ptr(asg), _ffi.ptr(out),
                                                    _ffi.ptr(ws), wsz, _ffi.stream_of(z)),
                   "rpc_anchor_head_loss_forward")
        ctx.save_for_backward(z, bias, asg, out, gb, ws, tab)
        ctx.cfg, ctx.M, ctx.wsz, ctx.layout = cfg, M, wsz, layout
        ctx.mark_non_differentiable(asg)
        # no zero-filled gradients for the assignment / positive count (a [B, H*W*A] memset per step)
        ctx.set_materialize_grads(False)
        return out[:3], asg, out[3:]

    @staticmethod
    def backward(ctx, g, _g_asg, _g_npos):
        lib = _ffi.load()
        z, bias, asg, out, gb, ws, tab = ctx.saved_tensors
        cfg = ctx.cfg
        g = (g if g is not None else torch.zeros(3, device=z.device)).float().contiguous()
        dz = torch.empty_like(z)
        N = bias.numel()
        db = torch.empty(N, dtype=torch.float32, device=z.device)
        _ffi.check(lib.rpc_anchor_head_loss_backward(C.byref(cfg), _ffi.ptr(tab), _ffi.ptr(gb), ctx.M, _ffi.ptr(z),
                                                     _ffi.ptr(bias), _ffi.ptr(asg), _ffi.ptr(g), _ffi.ptr(out),
                                                     _ffi.ptr(dz), _ffi.ptr(db), _ffi.ptr(ws), ctx.wsz,
                                                     _ffi.stream_of(z)), "rpc_anchor_head_loss_backward")
        return dz, db, None, None, None, None


class HeadLosses(dict):
    """upstream's dict of lists; `.packed` is the device [3] vector the entries view."""
    packed = None


class Anchor3DHead(nn.Module):
    def __init__(self, num_classes, in_channels, feat_channels=256, use_direction_classifier=True,
                 anchor_generator=dict(type="Anchor3DRangeGenerator", range=[0, -39.68, -1.78, 69.12, 39.68, -1.78],
                                       strides=[2], sizes=[[3.9, 1.6, 1.56]], rotations=[0, 1.57],
                                       custom_values=[], reshape_out=False),
                 assigner_per_size=False, assign_per_class=False, diff_rad_by_sin=True, dir_offset=-np.pi / 2,
                 dir_limit_offset=0, bbox_coder=dict(type="DeltaXYZWLHRBBoxCoder"),
                 loss_cls=dict(type="mmdet.CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type="mmdet.SmoothL1Loss", beta=1.0 / 9.0, loss_weight=2.0),
                 loss_dir=dict(type="mmdet.CrossEntropyLoss", loss_weight=0.2), train_cfg=None, test_cfg=None,
                 init_cfg=None):
        super().__init__()
        self.num_classes = num_classes
        self.in_channels = in_channels
        self.feat_channels = feat_channels
        self.use_direction_classifier = use_direction_classifier
        self.diff_rad_by_sin = diff_rad_by_sin
        self.dir_offset = dir_offset
        self.dir_limit_offset = dir_limit_offset
        self.assign_per_class = assign_per_class
        ag = dict(anchor_generator)
        ag.pop("type", None)
        ag.pop("strides", None)
        ag.pop("_delete_", None)
        if "range" in ag:
            ag["ranges"] = [ag.pop("range")]
        self.prior_generator = Anchor3DRangeGenerator(**ag)
        self.num_anchors = self.prior_generator.num_base_anchors
        self.bbox_coder = DeltaXYZWLHRBBoxCoder()
        self.box_code_size = self.bbox_coder.code_size
        self.loss_cls_cfg = dict(loss_cls)
        self.loss_bbox_cfg = dict(loss_bbox)
        self.loss_dir_cfg = dict(loss_dir)
        self.use_sigmoid_cls = loss_cls.get("use_sigmoid", False)
        self.sampling = loss_cls["type"] not in ["mmdet.FocalLoss", "mmdet.GHMC"]
        if self.sampling:
            raise NotImplementedError("only the sampling-free (FocalLoss) configuration is built")
        self.train_cfg = train_cfg or {}
        if self.train_cfg.get("code_weight"):
            raise NotImplementedError("train_cfg.code_weight is not used by the SECOND configs and not built")
        self.test_cfg = test_cfg
        assigners = self.train_cfg.get("assigner", None)
        if assigners is None:
            assigners = dict(pos_iou_thr=0.6, neg_iou_thr=0.45, min_pos_iou=0.45)
        self.assigners = assigners if isinstance(assigners, (list, tuple)) else [assigners]
        self.assigner_is_list = isinstance(assigners, (list, tuple))
        self.cls_out_channels = self.num_anchors * self.num_classes
        self.conv_cls = nn.Conv2d(self.feat_channels, self.cls_out_channels, 1)
        self.conv_reg = nn.Conv2d(self.feat_channels, self.num_anchors * self.box_code_size, 1)
        if use_direction_classifier:
            self.conv_dir_cls = nn.Conv2d(self.feat_channels, self.num_anchors * 2, 1)
        # init_cfg: Normal(std=0.01) on Conv2d, conv_cls bias prior 0.01
        for m in self._convs():
            nn.init.normal_(m.weight, 0.0, 0.01)
            nn.init.zeros_(m.bias)
        nn.init.constant_(self.conv_cls.bias, float(-np.log((1 - 0.01) / 0.01)))
        self._anchor_cache = {}
        self._tab_cache = {}

    def _convs(self):
        return [self.conv_cls, self.conv_reg] + ([self.conv_dir_cls] if self.use_direction_classifier else [])

    def _stacked(self):
        convs = self._convs()
        return torch.cat([c.weight for c in convs], 0), torch.cat([c.bias for c in convs], 0)

    # ------------------------------------------------------------------ head outputs
    def _z(self, x, w=None):
        """(z, layout, N): the stacked 1x1 conv WITHOUT bias as the HIP GEMM image [B*H*W, pad]:
        bf16 input -> the bf16 engine (pad HEAD_PAD); fp32 input -> the fp32 engine (pad
        head_pad_f32(N)). w: the stacked weight when the caller already built it."""
        if w is None:
            w, _ = self._stacked()
        N = w.shape[0]
        B, _, H, W = x.shape
        if not x.is_cuda:
            raise RuntimeError("Anchor3DHead runs on the HIP kernels only (no CPU path)")
        if x.dtype == torch.bfloat16:
            z = HeadConvFn.apply(x, w)
            return z, dict(B=B, H=H, W=W, bf16=1, sb=H * W * HEAD_PAD, shw=HEAD_PAD, sn=1, nwrite=HEAD_PAD), N
        NP = head_pad_f32(N)
        with torch.autocast("cuda", enabled=False):
            z = HeadConvF32Fn.apply(x.float(), w.float())
        return z, dict(B=B, H=H, W=W, bf16=0, sb=H * W * NP, shw=NP, sn=1, nwrite=NP), N

    def forward_single(self, x):
        w, b = self._stacked()
        z, lay, N = self._z(x, w)
        y = (z[:, :N].float() + b.float()).view(lay["B"], lay["H"], lay["W"], N).permute(0, 3, 1, 2)
        A = self.num_anchors
        outs = torch.split(y, [A * self.num_classes, A * 7] + ([A * 2] if self.use_direction_classifier else []),
                           dim=1)
        return outs[0], outs[1], (outs[2] if self.use_direction_classifier else None)

    def forward(self, feats):
        outs = [self.forward_single(x) for x in feats]
        return tuple(list(z) for z in zip(*outs))

    # ------------------------------------------------------------------ anchors / kernel config
    def anchors(self, featmap_size, device):
        key = (tuple(featmap_size), str(device))
        if key not in self._anchor_cache:
            self._anchor_cache[key] = self.prior_generator.grid_anchors([featmap_size], device)[0]
        return self._anchor_cache[key]

    def _kernel_cfg(self, lay, device):
        g = self.prior_generator
        S, R = len(g.ranges), len(g.rotations)
        key = (lay["H"], lay["W"], str(device))
        if key not in self._tab_cache:
            self._tab_cache[key] = anchor_table(g, lay["H"], lay["W"]).to(device)
        c = _ffi.RpcHeadCfg()
        c.B, c.H, c.W, c.S, c.R, c.C = lay["B"], lay["H"], lay["W"], S, R, self.num_classes
        per_size = self.assigner_is_list
        if per_size and len(self.assigners) != S:
            raise RuntimeError(f"{len(self.assigners)} assigners for {S} anchor sizes")
        c.NA = S if per_size else 1
        c.assigner_per_size, c.assign_per_class = int(per_size), int(self.assign_per_class)
        c.use_dir, c.diff_rad_by_sin = int(self.use_direction_classifier), int(self.diff_rad_by_sin)
        for i, a in enumerate(self.assigners[:c.NA]):
            c.pos_iou_thr[i], c.neg_iou_thr[i], c.min_pos_iou[i] = a["pos_iou_thr"], a["neg_iou_thr"], a["min_pos_iou"]
        c.dir_offset, c.dir_limit_offset = self.dir_offset, self.dir_limit_offset
        c.pos_weight = float(self.train_cfg.get("pos_weight", -1))
        c.beta = self.loss_bbox_cfg.get("beta", 1.0 / 9.0)
        c.gamma, c.alpha = self.loss_cls_cfg.get("gamma", 2.0), self.loss_cls_cfg.get("alpha", 0.25)
        c.lw_cls = self.loss_cls_cfg.get("loss_weight", 1.0)
        c.lw_bbox = self.loss_bbox_cfg.get("loss_weight", 2.0)
        c.lw_dir = self.loss_dir_cfg.get("loss_weight", 0.2)
        c.z_bf16, c.z_sb, c.z_shw, c.z_sn = lay["bf16"], lay["sb"], lay["shw"], lay["sn"]
        c.dz_bf16, c.dz_sb, c.dz_shw, c.dz_sn, c.dz_nwrite = lay["bf16"], lay["sb"], lay["shw"], lay["sn"], lay["nwrite"]
        return c, self._tab_cache[key]

    # ------------------------------------------------------------------ losses
    def loss_from_z(self, z, bias, lay, gt_boxes, gt_labels):
        """dict of LISTS like upstream loss_by_feat (one feature level)."""
        l3, asg, npos = HeadLossFn.apply(z, bias, self, lay, gt_boxes, gt_labels)
        self._last_assigned, self._last_num_total_pos = asg, npos
        out = HeadLosses(loss_cls=[l3[0]], loss_bbox=[l3[1]])
        if self.use_direction_classifier:
            out["loss_dir"] = [l3[2]]
            out.packed = l3   # [loss_cls, loss_bbox, loss_dir] on the device (fused loss tail)
        return out

    def loss(self, x, batch_data_samples):
        """x: tuple/list with one feature map [B, C, H, W]; batch_data_samples: dict(gt_boxes [B, M, 7],
        gt_labels [B, M]) or a list of per-image (boxes [Mi, 7], labels [Mi])."""
        feat = x[0]
        if not feat.is_cuda:
            raise RuntimeError("Anchor3DHead.loss runs on the HIP kernels only (no CPU path)")
        gb, gl = pack_gt(batch_data_samples, feat.device)
        w, b = self._stacked()
        z, lay, _ = self._z(feat, w)
        return self.loss_from_z(z, b, lay, gb, gl)

    # ------------------------------------------------------------------ detections
    @torch.no_grad()
    def predict_by_feat(self, cls_scores, bbox_preds, dir_cls_preds, cfg=None):
        """Detections from the head maps (one level; each a tensor [B, A*C | A*7 | A*2, H, W] or a one-element
        list): upstream `_predict_by_feat_single` + `box3d_multiclass_nms`, restated and batched. Per frame the
        `nms_pre` anchors of the largest max-class score are decoded; per class the candidates above `score_thr`
        go through rotated NMS at `nms_thr` in score order (a box may survive under several classes); the
        classes are concatenated (class-major, by score within a class) and cut to the `max_num` best scores;
        the direction bin corrects the yaw of the survivors. All frames x classes are ONE rpc_nms_bev call
        (postprocess.py); the only device -> host transfer is of the final per-frame counts.
        -> per frame dict(bboxes_3d [n, 7], scores_3d [n], labels_3d [n] int64)."""
        from . import postprocess as pp
        one = lambda v: v[0] if isinstance(v, (list, tuple)) else v
        cls, reg, dcl = one(cls_scores), one(bbox_preds), one(dir_cls_preds)
        cfg = dict(self.test_cfg or {}) if cfg is None else dict(cfg)
        if not cfg.get("use_rotate_nms", True):
            raise NotImplementedError("test_cfg.use_rotate_nms=False (axis-aligned BEV NMS) is not built")
        B, _, H, W = cls.shape
        C_, A = self.num_classes, self.num_anchors
        g = self.prior_generator
        S, R = len(g.ranges), len(g.rotations)
        N = H * W * A
        dev = cls.device
        key = (H, W, str(dev))
        if key not in self._tab_cache:
            self._tab_cache[key] = anchor_table(g, H, W).to(dev)
        nms_pre = int(cfg.get("nms_pre", -1))
        if 0 < nms_pre < N:
            best = torch.sigmoid(cls.float().reshape(B, A, C_, H, W).amax(2)).permute(0, 2, 3, 1).reshape(B, N)
            cand = best.topk(nms_pre, dim=1)[1]
        else:
            cand = torch.arange(N, device=dev)[None].expand(B, N)
        K = cand.shape[1]
        scores, boxes, dirl = pp.anchor_decode(cand, cls, reg, dcl, self._tab_cache[key], S, R, C_)
        # groups = frames x classes: each class's candidates in score order at the front of its group
        sc = scores.permute(0, 2, 1)                                            # [B, C, K]
        cand_ok = sc > float(cfg.get("score_thr", 0.0))
        order = torch.sort(sc.masked_fill(~cand_ok, -1.0), dim=2, descending=True, stable=True)[1]
        counts = cand_ok.sum(2)
        bev = torch.cat([boxes[..., 0:2], boxes[..., 3:5], boxes[..., 6:7]], -1)   # x, y, dx, dy, yaw
        bev = bev[:, None].expand(B, C_, K, 5).gather(2, order[..., None].expand(-1, -1, -1, 5))
        keep, nkeep = pp.nms_bev_batched(bev.reshape(B * C_, K, 5), counts.reshape(-1), float(cfg["nms_thr"]))
        keep, nkeep = keep.view(B, C_, K).long(), nkeep.view(B, C_, 1)
        kept = torch.arange(K, device=dev)[None, None] < nkeep
        src = order.gather(2, keep.clamp(min=0))                                # candidate of each kept slot
        ksc = sc.gather(2, src).masked_fill(~kept, -1.0).reshape(B, C_ * K)
        kept, src = kept.reshape(B, C_ * K), src.reshape(B, C_ * K)
        total = kept.sum(1)
        max_num = int(cfg.get("max_num", C_ * K))
        M = min(max_num, C_ * K)
        by_class = pp.compact_front(kept)[0]
        by_score = torch.sort(ksc, dim=1, descending=True, stable=True)[1]
        sel = torch.where((total > max_num)[:, None], by_score, by_class)[:, :M]
        src = src.gather(1, sel)
        out_b = boxes.gather(1, src[..., None].expand(-1, -1, 7)).clone()
        out_s = ksc.gather(1, sel)
        out_l = sel // K
        if self.use_direction_classifier and dcl is not None:
            rot = limit_period(out_b[..., 6] - self.dir_offset, self.dir_limit_offset, math.pi)
            out_b[..., 6] = rot + self.dir_offset + math.pi * dirl.gather(1, src).to(out_b.dtype)
        n = total.clamp(max=M).tolist()                                         # the one device -> host transfer
        return [dict(bboxes_3d=out_b[b, :n[b]], scores_3d=out_s[b, :n[b]], labels_3d=out_l[b, :n[b]])
                for b in range(B)]


def pack_gt(samples, device):
    """GT of one batch -> padded (boxes [B, M, 7] fp32, labels [B, M] int64, -1 padding). `samples`:
    the trainer's dict(gt_boxes, gt_labels); mmdet3d Det3DDataSamples (what Anchor3DHead.loss
    receives from AdversarialVoxelNet.loss, adversarial_voxelnet.py:168 — duck-typed
    `gt_instances_3d.bboxes_3d(.tensor)` / `.labels_3d`); or (boxes, labels) pairs."""
    if isinstance(samples, dict):
        return samples["gt_boxes"].to(device), samples["gt_labels"].to(device)
    d = det3d_gt(samples)
    if d is not None:
        samples = [(b[:, :7], l) for b, l in zip(*d)]
    M = max(1, max(int(b.shape[0]) for b, _ in samples))
    B = len(samples)
    dev_t = torch.device(device).type
    if dev_t != "cpu" and all(torch.is_tensor(b) and b.device.type == dev_t for b, _ in samples):
        # already on the device (mmdet3d's data preprocessor moved the samples): pad there, no host copy
        boxes = torch.zeros((B, M, 7), dtype=torch.float32, device=device)
        labels = torch.full((B, M), -1, dtype=torch.long, device=device)
        for i, (b, l) in enumerate(samples):
            n = int(b.shape[0])
            if n:
                boxes[i, :n] = b.float()
                labels[i, :n] = torch.as_tensor(l, device=device).long()
        boxes[..., 3:6] = torch.where(labels[..., None] >= 0, boxes[..., 3:6], torch.ones_like(boxes[..., 3:6]))
        return boxes, labels
    boxes = torch.zeros((B, M, 7), dtype=torch.float32)
    labels = torch.full((B, M), -1, dtype=torch.long)
    for i, (b, l) in enumerate(samples):
        n = int(b.shape[0])
        boxes[i, :n] = torch.as_tensor(b, dtype=torch.float32)
        labels[i, :n] = torch.as_tensor(l, dtype=torch.long)
    # padded boxes get unit size so the encoder never divides by zero (they are masked)
    boxes[..., 3:6] = torch.where(labels[..., None] >= 0, boxes[..., 3:6], torch.ones_like(boxes[..., 3:6]))
    return boxes.to(device, non_blocking=True), labels.to(device, non_blocking=True)
