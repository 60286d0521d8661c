"""Detection post-processing behind `predict`: rotated-BEV NMS, circle NMS and box decoding.

Restates upstream mmdet3d v1.x `nms_bev` / `circle_nms` (models/layers/box3d_nms.py) over mmcv
`nms_rotated`, `DeltaXYZWLHRBBoxCoder.decode` and `CenterPointBBoxCoder.decode`. CUDA tensors run on the HIP
kernels of csrc/postprocess.hip (`rpc_nms_bev`, `rpc_nms_circle`, `rpc_bev_iou_pairs`, `rpc_anchor_decode`,
`rpc_center_decode`), batched over groups (frames x classes, frames x tasks) with the per-group counts kept on
the device; ordering by score and top-k selection are torch.sort / torch.topk. CPU tensors take a plain
Python / torch path with the same semantics (slow; it makes `predict` usable and testable without a GPU, like
the torch paths of second.py). The heads' `predict_by_feat` (anchor_head.py, center_head.py) use the batched
forms; `nms_bev` and `circle_nms` are the single-set forms of mmdet3d.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _ffi

__all__ = ["bev_iou_pairs", "nms_bev", "circle_nms", "nms_bev_batched", "nms_circle_batched", "anchor_decode",
           "center_decode", "compact_front"]


# ----------------------------------------------------------------------------------- CPU path
def _iou_cpu(a, b) -> float:
    """IoU of two (x, y, dx, dy, yaw) boxes in Python floats, the construction of csrc/bev_iou.h: b in the
    frame of a, clipped against a's four sides."""
    ax, ay, adx, ady, ar = a
    bx, by, bdx, bdy, br = b
    if not (adx > 0 and ady > 0 and bdx > 0 and bdy > 0):
        return 0.0
    ca, sa = math.cos(ar), math.sin(ar)
    tx, ty = bx - ax, by - ay
    cx, cy = ca * tx + sa * ty, ca * ty - sa * tx
    cd, sd = math.cos(br - ar), math.sin(br - ar)
    ux, uy, vx, vy = cd * bdx / 2, sd * bdx / 2, -sd * bdy / 2, cd * bdy / 2
    poly = [(cx + ux + vx, cy + uy + vy), (cx - ux + vx, cy - uy + vy), (cx - ux - vx, cy - uy - vy),
            (cx + ux - vx, cy + uy - vy)]
    for axis, sgn, lim in ((0, 1, adx / 2), (0, -1, adx / 2), (1, 1, ady / 2), (1, -1, ady / 2)):
        out = []
        for k in range(len(poly)):
            p, q = poly[k - 1], poly[k]
            dp, dq = sgn * p[axis] - lim, sgn * q[axis] - lim
            if (dp <= 0) != (dq <= 0):
                t = dp / (dp - dq)
                o = p[1 - axis] + t * (q[1 - axis] - p[1 - axis])
                out.append((sgn * lim, o) if axis == 0 else (o, sgn * lim))
            if dq <= 0:
                out.append(q)
        poly = out
        if not poly:
            return 0.0
    s = 0.0
    for k in range(len(poly)):
        s += (poly[k - 1][0] - poly[k][0]) * (poly[k - 1][1] + poly[k][1])
    area_a, area_b = adx * ady, bdx * bdy
    inter = min(abs(s) / 2, area_a, area_b)
    iou = inter / (area_a + area_b - inter)
    return min(iou, 1.0) if iou >= 0 else 0.0


def _greedy_cpu(n, max_keep, suppresses):
    removed = [False] * n
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        if len(keep) >= max_keep:
            break
        keep.append(i)
        for j in range(i + 1, n):
            if not removed[j] and suppresses(i, j):
                removed[j] = True
    return keep


def _nms_cpu(rows, counts, max_keep, make_pred):
    G, N = rows.shape[:2]
    keep = torch.full((G, max_keep), -1, dtype=torch.int32)
    nkeep = torch.zeros(G, dtype=torch.int32)
    for g in range(G):
        n = min(max(int(counts[g]), 0), N)
        k = _greedy_cpu(n, max_keep, make_pred(g, rows[g].tolist()))
        keep[g, :len(k)] = torch.tensor(k, dtype=torch.int32)
        nkeep[g] = len(k)
    return keep, nkeep


# ----------------------------------------------------------------------------------- kernels
def bev_iou_pairs(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """IoU of the rotated BEV boxes a[i], b[i] ([n, 5] each: x, y, dx, dy, yaw) -> [n] fp32."""
    a = a.float().contiguous().reshape(-1, 5)
    b = b.float().contiguous().reshape(-1, 5)
    if a.shape != b.shape:
        raise ValueError("bev_iou_pairs needs two [n, 5] box sets of one size")
    n = a.shape[0]
    if not a.is_cuda:
        return torch.tensor([_iou_cpu(x, y) for x, y in zip(a.tolist(), b.tolist())], dtype=torch.float32)
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    _ffi.check(_ffi.load().rpc_bev_iou_pairs(_ffi.ptr(a), _ffi.ptr(b), n, _ffi.ptr(out), _ffi.stream_of(a)),
               "rpc_bev_iou_pairs")
    return out


def _nms_hip(entry, what, rows, counts, radius, thr, max_keep):
    lib = _ffi.load()
    G, N = rows.shape[:2]
    dev = rows.device
    keep = torch.empty((G, max_keep), dtype=torch.int32, device=dev)
    nkeep = torch.empty(G, dtype=torch.int32, device=dev)
    wsz = lib.rpc_nms_workspace_size(G, N)
    ws = _ffi.workspace(wsz, dev)
    args = (_ffi.ptr(rows), _ffi.ptr(counts)) + ((_ffi.ptr(radius),) if radius is not None else ()) + (G, N)
    args += ((float(thr),) if radius is None else ()) + (max_keep, _ffi.ptr(keep), _ffi.ptr(nkeep), _ffi.ptr(ws), wsz,
                                                         _ffi.stream_of(rows))
    _ffi.check(entry(*args), what)
    return keep, nkeep


def nms_bev_batched(boxes5: torch.Tensor, counts: torch.Tensor, thr: float, max_keep: int | None = None):
    """Greedy rotated NMS of G groups in one call. boxes5 [G, N, 5] sorted within each group by descending
    score, counts [G] (boxes of each group that take part). -> keep [G, max_keep] int32 (indices into the
    group in score order, -1 padding), nkeep [G] int32. Box j is suppressed by a kept i < j when
    IoU(i, j) > thr. N is capped at _ffi.NMS_MAX_N on the device."""
    G, N = boxes5.shape[:2]
    max_keep = N if max_keep is None else min(int(max_keep), N)
    boxes5 = boxes5.float().contiguous()
    counts = counts.to(torch.int32).contiguous()
    if boxes5.is_cuda:
        return _nms_hip(_ffi.load().rpc_nms_bev, "rpc_nms_bev", boxes5, counts, None, thr, max_keep)
    thr = float(thr)
    return _nms_cpu(boxes5, counts, max_keep, lambda g, b: (lambda i, j: _iou_cpu(b[i], b[j]) > thr))


def nms_circle_batched(xy: torch.Tensor, counts: torch.Tensor, radius: torch.Tensor, max_keep: int | None = None):
    """Greedy centre-distance NMS of G groups in one call: xy [G, N, 2] in score order, counts [G],
    radius [G]. Box j is suppressed by a kept i < j when dx*dx + dy*dy <= radius[g]: mmdet3d's circle_nms
    compares the SQUARED distance with the UNSQUARED min_radius, non-strictly; kept for parity."""
    G, N = xy.shape[:2]
    max_keep = N if max_keep is None else min(int(max_keep), N)
    xy = xy.float().contiguous()
    counts = counts.to(torch.int32).contiguous()
    radius = radius.to(device=xy.device, dtype=torch.float32).contiguous()
    if xy.is_cuda:
        return _nms_hip(_ffi.load().rpc_nms_circle, "rpc_nms_circle", xy, counts, radius, None, max_keep)
    f32 = torch.float32
    d = xy[:, :, None, :] - xy[:, None, :, :]          # fp32 like the kernel: dx*dx + dy*dy, no fused multiply-add
    hit = ((d[..., 0] * d[..., 0]).to(f32) + (d[..., 1] * d[..., 1]).to(f32) <= radius[:, None, None]).tolist()
    return _nms_cpu(xy, counts, max_keep, lambda g, _: (lambda i, j: hit[g][i][j]))


def nms_bev(boxes5, scores, thr, pre_max_size=None, post_max_size=None):
    """mmdet3d `nms_bev`: rotated NMS of one box set ([n, 5]: x, y, dx, dy, yaw) -> kept indices (int64, by
    descending score)."""
    order = scores.sort(0, descending=True)[1]
    if pre_max_size is not None:
        order = order[:pre_max_size]
    n = int(order.numel())
    if n == 0:
        return order
    counts = torch.full((1,), n, dtype=torch.int32, device=boxes5.device)
    keep, nkeep = nms_bev_batched(boxes5[order][None], counts, thr)
    keep = order[keep[0, :int(nkeep[0])].long()]
    return keep[:post_max_size] if post_max_size is not None else keep


def circle_nms(xy, scores, radius, post_max_size=None):
    """mmdet3d `circle_nms` of one set of centres ([n, 2]) -> kept indices (int64, by descending score)."""
    order = scores.sort(0, descending=True)[1]
    n = int(order.numel())
    if n == 0:
        return order
    counts = torch.full((1,), n, dtype=torch.int32, device=xy.device)
    rad = torch.full((1,), float(radius), dtype=torch.float32, device=xy.device)
    keep, nkeep = nms_circle_batched(xy[order][None], counts, rad, post_max_size)
    return order[keep[0, :int(nkeep[0])].long()]


def anchor_decode(cand, cls, reg, dcl, table, S, R, num_classes):
    """Candidate anchors of the Anchor3DHead maps. cand [B, K] flat anchor indices (((h*W + w)*S + s)*R + r),
    cls [B, A*C, H, W], reg [B, A*7, H, W], dcl [B, A*2, H, W] or None (any strides), table: anchor_table.
    -> scores [B, K, C] (sigmoid), boxes [B, K, 7] (DeltaXYZWLHRBBoxCoder.decode), dir label [B, K]."""
    B, _, H, W = cls.shape
    K = cand.shape[1]
    Cn = num_classes
    A = S * R
    cls, reg = cls.float(), reg.float()
    dcl = None if dcl is None else dcl.float()
    if cls.is_cuda:
        dev = cls.device
        cand = cand.to(torch.int32).contiguous()
        scores = torch.empty((B, K, Cn), dtype=torch.float32, device=dev)
        boxes = torch.empty((B, K, 7), dtype=torch.float32, device=dev)
        dirl = torch.empty((B, K), dtype=torch.int32, device=dev)
        st = list(cls.stride()) + list(reg.stride()) + (list(dcl.stride()) if dcl is not None else [0] * 4)
        _ffi.check(_ffi.load().rpc_anchor_decode(_ffi.ptr(cand), B, K, H, W, S, R, Cn, _ffi.ptr(table), _ffi.ptr(cls),
                                                 _ffi.ptr(reg), _ffi.ptr(dcl), (C.c_longlong * 12)(*st),
                                                 _ffi.ptr(scores), _ffi.ptr(boxes), _ffi.ptr(dirl),
                                                 _ffi.stream_of(cls)), "rpc_anchor_decode")
        return scores, boxes, dirl.long()
    cand = cand.long()
    r, s = cand % R, (cand // R) % S
    w, h = (cand // A) % W, cand // (A * W)
    xc, yc, zc, sz, rot = torch.split(table.float(), [S * W, S * H, S, 3 * S, R])
    sz = sz.view(S, 3)
    anchors = torch.stack([xc[s * W + w], yc[s * H + h], zc[s], sz[s, 0], sz[s, 1], sz[s, 2], rot[r]], -1)

    def rows(m, n):   # [B, A*n, H, W] -> the candidates' [B, K, n]
        return m.permute(0, 2, 3, 1).reshape(B, H * W * A, n).gather(1, cand[..., None].expand(-1, -1, n))

    from .anchor_head import DeltaXYZWLHRBBoxCoder
    boxes = DeltaXYZWLHRBBoxCoder.decode(anchors, rows(reg, 7))
    dirl = torch.zeros((B, K), dtype=torch.long) if dcl is None else rows(dcl, 2).max(-1)[1]
    return torch.sigmoid(rows(cls, Cn)), boxes, dirl


def center_decode(hm, box, topk, task_ncls, task_k, B, H, W, norm_bbox, out_size_factor, voxel_size, pc_range,
                  score_threshold, limit):
    """Top-K cells of the CenterHead's packed buffers hm [B*H*W, hm_pitch], box [B*H*W, box_pitch]; topk
    [B, T, K] indices into each task's [ncls, H, W] scores (entries >= task_k[t] are padding).
    -> boxes [B, T, K, 9] (x, y, z centre, dim, rot, vel), scores, labels (within the task), valid (bool)."""
    T, K = topk.shape[1:]
    hm = hm.float().contiguous().view(B * H * W, -1)
    box = box.float().contiguous().view(B * H * W, -1)
    if hm.is_cuda:
        dev = hm.device
        c = _ffi.RpcCenterDecodeCfg()
        c.B, c.H, c.W, c.K, c.ntasks = B, H, W, K, T
        for t in range(T):
            c.task_ncls[t], c.task_k[t] = task_ncls[t], task_k[t]
        c.hm_pitch, c.box_pitch = hm.shape[1], box.shape[1]
        c.norm_bbox, c.out_size_factor = int(bool(norm_bbox)), int(out_size_factor)
        c.use_score_threshold = int(score_threshold is not None)
        c.score_threshold = float(score_threshold or 0.0)
        c.voxel_x, c.voxel_y, c.pc_x, c.pc_y = voxel_size[0], voxel_size[1], pc_range[0], pc_range[1]
        for k in range(6):
            c.limit[k] = float(limit[k])
        topk = topk.to(torch.int32).contiguous()
        boxes = torch.empty((B, T, K, 9), dtype=torch.float32, device=dev)
        scores = torch.empty((B, T, K), dtype=torch.float32, device=dev)
        labels = torch.empty((B, T, K), dtype=torch.int32, device=dev)
        valid = torch.empty((B, T, K), dtype=torch.int32, device=dev)
        _ffi.check(_ffi.load().rpc_center_decode(C.byref(c), _ffi.ptr(hm), _ffi.ptr(box), _ffi.ptr(topk),
                                                 _ffi.ptr(boxes), _ffi.ptr(scores), _ffi.ptr(labels), _ffi.ptr(valid),
                                                 _ffi.stream_of(hm)), "rpc_center_decode")
        return boxes, scores, labels.long(), valid.bool()
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)
    outs = []
    c0 = 0
    frame = torch.arange(B)[:, None] * (H * W)
    for t in range(T):
        idx = topk[:, t].long()
        cls, cell = idx // (H * W), idx % (H * W)
        p = frame + cell
        v = box[p][..., 10 * t:10 * t + 10]
        score = torch.sigmoid(hm[p, c0 + cls])
        x = (cell % W + v[..., 0]) * f(out_size_factor) * f(voxel_size[0]) + f(pc_range[0])
        y = (cell // W + v[..., 1]) * f(out_size_factor) * f(voxel_size[1]) + f(pc_range[1])
        z = v[..., 2]
        dim = torch.exp(v[..., 3:6]) if norm_bbox else v[..., 3:6]
        rot = torch.atan2(v[..., 6], v[..., 7])
        ok = torch.arange(K)[None, :] < task_k[t]
        if score_threshold is not None:
            ok = ok & (score > f(score_threshold))
        for q, lo, hi in ((x, limit[0], limit[3]), (y, limit[1], limit[4]), (z, limit[2], limit[5])):
            ok = ok & (q >= f(lo)) & (q <= f(hi))
        outs.append((torch.cat([x[..., None], y[..., None], z[..., None], dim, rot[..., None], v[..., 8:10]], -1),
                     score, cls, ok))
        c0 += task_ncls[t]
    return tuple(torch.stack([o[k] for o in outs], 1) for k in range(4))


def compact_front(flag: torch.Tensor):
    """Per row of flag [..., N] (bool): (order, count) with order the stable permutation that moves the set
    entries to the front, count their number."""
    order = torch.sort((~flag).to(torch.uint8), dim=-1, stable=True)[1]
    return order, flag.sum(-1)
