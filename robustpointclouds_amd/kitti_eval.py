"""KITTI average precision (BEV and 3D, R11 and R40) from the per-frame dicts `predict` returns.

Restates mmdet3d v1.x `evaluation/functional/kitti_utils/eval.py` (`clean_data`, `compute_statistics_jit`,
`get_thresholds`, `eval_class`, `get_mAP11/40`) in the LiDAR frame; the specification is written out in
DESIGN.md "KITTI average precision". Boxes are LiDAR boxes (x, y, z of the BOTTOM face, dx, dy, dz, yaw) as
`predict` returns them; of a 9-column CenterPoint box the first 7 columns are used.

With a camera calibration (`read_calib`, `lidar2img`; the ground-truth dicts' `lidar2img` / `img_shape`) the boxes
are projected into the image (DESIGN.md "Calibration"; mmdet3d `KittiMetric.convert_valid_bboxes`,
`bbox2result_kitti`): detections outside the image or `pcd_limit_range` are removed, the pixel heights make the
three difficulties differ, and `metrics=("BEV", "3D", "2D", "AOS")` adds the 2D `bbox` metric (with DontCare
regions) and the orientation similarity. On CUDA tensors that is `rpc_kitti_project`, `rpc_kitti_overlaps_2d` and
`rpc_kitti_match_counts_aos`, with no host read beyond the two below.

CUDA tensors run on the HIP kernels of csrc/kitti_eval.hip — `rpc_kitti_overlaps` (all frames' overlap
matrices in one launch), `rpc_kitti_match_scores` (matcher pass 1) and `rpc_kitti_match_counts` (pass 2, one
lane per threshold) — with one host read between the passes (how many scores each group emitted: the positions
of the thresholds in the sorted scores depend on nothing else) and one at the end (the counts). CPU tensors
take a plain Python / torch path with the same semantics (slow; like postprocess.py's, it makes the metric
usable and testable without a GPU). Sorting, flags, precision and AP are torch on either path.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _ffi
from .postprocess import _iou_cpu

__all__ = ["box_overlaps", "threshold_indices", "KittiAP", "DIFFICULTIES", "MIN_HEIGHT", "MAX_OCCLUSION",
           "MAX_TRUNCATION", "MIN_OVERLAP_STRICT", "MIN_OVERLAP_LOOSE", "read_calib", "lidar2img", "project_boxes",
           "box_overlaps_2d", "ALL_METRICS", "PCD_LIMIT_RANGE"]

DIFFICULTIES = ("easy", "moderate", "hard")
MIN_HEIGHT = (40.0, 25.0, 25.0)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
MIN_OVERLAP_STRICT = {"Car": 0.7, "Pedestrian": 0.5, "Cyclist": 0.5}
MIN_OVERLAP_LOOSE = {"Car": 0.5, "Pedestrian": 0.25, "Cyclist": 0.25}
TABLES = ("strict", "loose")
METRICS = ("BEV", "3D")
ALL_METRICS = ("BEV", "3D", "2D", "AOS")
PCD_LIMIT_RANGE = (0, -40, -3, 70.4, 40, 0.0)
NO = _ffi.KITTI_NO_SCORE
N_THR = _ffi.KITTI_MAX_THR
SIM_ONE = _ffi.KITTI_SIM_ONE


# ----------------------------------------------------------------------------------- calibration (host)
def read_calib(path) -> dict:
    """A KITTI `calib/*.txt` file -> {"P2": [3, 4], "R0_rect": [3, 3], "Tr_velo_to_cam": [3, 4]} float64 numpy
    arrays (other lines of the file are kept out). ValueError if one of the three is missing or of the wrong size."""
    shapes = {"P2": (3, 4), "R0_rect": (3, 3), "Tr_velo_to_cam": (3, 4)}
    out = {}
    with open(path) as f:
        for line in f:
            name, sep, rest = line.partition(":")
            if sep and name.strip() in shapes:
                vals = np.array(rest.split(), dtype=np.float64)
                shape = shapes[name.strip()]
                if vals.size != shape[0] * shape[1]:
                    raise ValueError(f"{path}: {name.strip()} has {vals.size} numbers, not {shape[0] * shape[1]}")
                out[name.strip()] = vals.reshape(shape)
    missing = [k for k in shapes if k not in out]
    if missing:
        raise ValueError(f"{path}: no {', '.join(missing)} line")
    return out


def lidar2img(P2, R0_rect, Tr_velo_to_cam) -> np.ndarray:
    """P2 . R0_rect . Tr_velo_to_cam -> [3, 4] fp32: R0_rect padded to a 4 x 4 block form, Tr_velo_to_cam given the
    fourth row (0, 0, 0, 1), the product formed in float64 and rounded to fp32 once."""
    P = np.asarray(P2, dtype=np.float64).reshape(3, 4)
    R = np.eye(4)
    R[:3, :3] = np.asarray(R0_rect, dtype=np.float64).reshape(3, 3)
    T = np.eye(4)
    T[:3, :4] = np.asarray(Tr_velo_to_cam, dtype=np.float64).reshape(3, 4)
    return (P @ R @ T).astype(np.float32)


# ----------------------------------------------------------------------------------- CPU path
def _overlap_cpu(a, b, mode) -> float:
    """Overlap of two 7-number boxes in Python floats, the construction of csrc/box_overlap.h (a is the
    clipper's rectangle; z relative to a's bottom face)."""
    if not (a[3] > 0 and a[4] > 0 and a[5] > 0 and b[3] > 0 and b[4] > 0 and b[5] > 0):
        return 0.0
    iou = _iou_cpu((a[0], a[1], a[3], a[4], a[6]), (b[0], b[1], b[3], b[4], b[6]))
    if mode == 0:
        return iou
    tz = b[2] - a[2]
    h = min(tz + b[5], a[5]) - max(tz, 0.0)
    if not h > 0:
        return 0.0
    area_a, area_b = a[3] * a[4], b[3] * b[4]
    area = iou * (area_a + area_b) / (1.0 + iou)        # the intersection area the IoU was formed from
    va, vb = area_a * a[5], area_b * b[5]
    inter = min(area * h, va, vb)
    v = inter / (va + vb - inter)
    return min(v, 1.0) if v >= 0 else 0.0


def _sim_fixed(alpha_gt, alpha_det) -> int:
    """(1 + cos(alpha_gt - alpha_det)) / 2 in float64, in units of 1 / SIM_ONE (the kernel's fixed point)."""
    v = (1.0 + math.cos(alpha_gt - alpha_det)) * 0.5 if math.isfinite(alpha_gt - alpha_det) else 0.0
    return int(round(min(max(v, 0.0), 1.0) * SIM_ONE))


def _match_frame(ov, score, fdet, fgt, min_ov, thresh, count_pass, stuff=None, alpha=None, sim=None):
    """compute_statistics_jit for one frame: ov[j][i] (lists), score / fdet per detection, fgt per ground
    truth. -> tp, fp, fn, {gt index: score of its true positive}. stuff (per detection): a stuff detection is no
    false positive. alpha = (per detection, per ground truth) and sim (a list): every true positive appends its
    orientation similarity in fixed point to sim."""
    nd = len(score)
    assigned = [False] * nd
    ignored_thr = [count_pass and score[j] < thresh for j in range(nd)]
    tp = fp = fn = 0
    emitted = {}
    for i, gf in enumerate(fgt):
        if gf == -1:
            continue
        det, valid, max_ov, took_ignored = -1, NO, 0.0, False
        for j in range(nd):
            if fdet[j] == -1 or assigned[j] or ignored_thr[j]:
                continue
            o = ov[j][i]
            if not count_pass and o > min_ov and score[j] > valid:
                det, valid = j, score[j]
            elif count_pass and o > min_ov and (o > max_ov or took_ignored) and fdet[j] == 0:
                max_ov, det, valid, took_ignored = o, j, 1, False
            elif count_pass and o > min_ov and valid == NO and fdet[j] == 1:
                det, valid, took_ignored = j, 1, True
        if valid == NO and gf == 0:
            fn += 1
        elif valid != NO and (gf == 1 or fdet[det] == 1):
            assigned[det] = True
        elif valid != NO:
            tp += 1
            emitted[i] = score[det]
            assigned[det] = True
            if alpha is not None and sim is not None:
                sim.append(_sim_fixed(alpha[1][i], alpha[0][det]))
    if count_pass:
        fp = sum(1 for j in range(nd) if not (assigned[j] or fdet[j] in (-1, 1) or ignored_thr[j]
                                              or (stuff is not None and stuff[j])))
    return tp, fp, fn, emitted


def _frames_cpu(ov, ov_off, det_off, gt_off, score, fdet_row, fgt_row):
    """Per frame: (ov as nested lists [nd][ng], scores, det flags, gt flags, first gt row)."""
    for f in range(len(det_off) - 1):
        d0, d1, g0, g1 = det_off[f], det_off[f + 1], gt_off[f], gt_off[f + 1]
        nd, ng = d1 - d0, g1 - g0
        o = ov[ov_off[f]:ov_off[f] + nd * ng].view(nd, ng).tolist() if nd and ng else [[] for _ in range(nd)]
        yield o, score[d0:d1], fdet_row[d0:d1], fgt_row[g0:g1], g0


# ----------------------------------------------------------------------------------- overlaps
def _offsets(counts):
    off = [0]
    for c in counts:
        off.append(off[-1] + int(c))
    return off


def _host_offsets(off):
    if isinstance(off, torch.Tensor):
        off = off.detach().cpu().tolist()
    off = [int(v) for v in off]
    if not off or off[0] != 0 or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError("offsets must start at 0 and not decrease")
    return off


def _check_caps(det_off, gt_off):
    maxd = max((b - a for a, b in zip(det_off, det_off[1:])), default=0)
    maxg = max((b - a for a, b in zip(gt_off, gt_off[1:])), default=0)
    if maxd > _ffi.KITTI_MAX_DET or maxg > _ffi.KITTI_MAX_GT:
        raise ValueError(f"a frame has {maxd} detections / {maxg} ground truths; the evaluator takes at most "
                         f"{_ffi.KITTI_MAX_DET} / {_ffi.KITTI_MAX_GT} per frame")
    return maxd, maxg


def _overlaps(det, det_off, gt, gt_off, ov_off, maxd, maxg, mode, dev_off=None):
    total = ov_off[-1]
    if not det.is_cuda:
        out = torch.zeros(total, dtype=torch.float32)
        dl, gl = det.tolist(), gt.tolist()
        vals = []
        for f in range(len(det_off) - 1):
            for j in range(det_off[f], det_off[f + 1]):
                vals += [_overlap_cpu(gl[i], dl[j], mode) for i in range(gt_off[f], gt_off[f + 1])]
        if vals:
            out = torch.tensor(vals, dtype=torch.float32)
        return out
    dev = det.device
    ov = torch.empty(total, dtype=torch.float32, device=dev)
    d_off, g_off, o_off = dev_off
    _ffi.check(_ffi.load().rpc_kitti_overlaps(_ffi.ptr(det), _ffi.ptr(d_off), _ffi.ptr(gt), _ffi.ptr(g_off),
                                              _ffi.ptr(o_off), len(det_off) - 1, maxd, maxg, mode, _ffi.ptr(ov),
                                              _ffi.stream_of(det)), "rpc_kitti_overlaps")
    return ov


def _device_offsets(det_off, gt_off, ov_off, dev):
    return (torch.tensor(det_off, dtype=torch.int32, device=dev), torch.tensor(gt_off, dtype=torch.int32, device=dev),
            torch.tensor(ov_off, dtype=torch.int64, device=dev))


def box_overlaps(dets: torch.Tensor, det_off, gts: torch.Tensor, gt_off, mode: int):
    """Overlap matrices of F frames in one call. dets [sum Nd, 7+], gts [sum Ng, 7+] LiDAR boxes (the first 7
    columns are used), det_off / gt_off [F + 1] host integers (a device tensor is read back), mode 0: rotated
    BEV IoU, 1: 3D IoU. -> (ov, ov_off): ov flat fp32 with frame f's [Nd, Ng] matrix at
    ov[ov_off[f] : ov_off[f + 1]], ov_off a list. Finite in [0, 1]; exactly 0 for any extent <= 0; exactly 1 for
    identical boxes. At most KITTI_MAX_DET / KITTI_MAX_GT boxes per frame (ValueError above)."""
    if mode not in (0, 1):
        raise ValueError("mode is 0 (BEV) or 1 (3D)")
    det_off, gt_off = _host_offsets(det_off), _host_offsets(gt_off)
    if len(det_off) != len(gt_off):
        raise ValueError("det_off and gt_off describe different numbers of frames")
    dets = dets.reshape(-1, dets.shape[-1])[:, :7].float().contiguous()
    gts = gts.reshape(-1, gts.shape[-1])[:, :7].float().contiguous().to(dets.device)
    if det_off[-1] != dets.shape[0] or gt_off[-1] != gts.shape[0]:
        raise ValueError("the offsets do not end at the number of boxes")
    maxd, maxg = _check_caps(det_off, gt_off)
    ov_off = _offsets([(det_off[f + 1] - det_off[f]) * (gt_off[f + 1] - gt_off[f]) for f in range(len(det_off) - 1)])
    dev_off = _device_offsets(det_off, gt_off, ov_off, dets.device) if dets.is_cuda else None
    return _overlaps(dets, det_off, gts, gt_off, ov_off, maxd, maxg, mode, dev_off), ov_off


# ----------------------------------------------------------------------------------- calibration (boxes)
def _frame_index(off, dev):
    """The frame of every row, from host offsets (no device read: the output size is known)."""
    counts = torch.tensor([b - a for a, b in zip(off, off[1:])], dtype=torch.int64, device=dev)
    return torch.repeat_interleave(torch.arange(len(off) - 1, device=dev), counts, output_size=off[-1])


def _project_cpu(box, off, mat, hw, rng):
    """The projection of DESIGN.md "Calibration" in torch fp32, every operation rounded in the kernel's order."""
    n, m = box.shape[0], off[-1]
    out = dict(raw=torch.zeros(n, 4), clip=torch.zeros(n, 4), valid=torch.zeros(n, dtype=torch.bool),
               alpha=torch.zeros(n, dtype=torch.float64), height=torch.zeros(n))
    if m == 0:
        return out
    fi = _frame_index(off, "cpu")
    M, H, W = mat[fi], hw[fi, 0], hw[fi, 1]
    x, y, z, dx, dy, dz, yaw = (box[:m, k] for k in range(7))
    s, c = torch.sin(yaw), torch.cos(yaw)
    hx, hy, zt = dx * 0.5, dy * 0.5, z + dz
    us, vs = [], []
    for k in range(8):
        lx, ly, cz = (-hx if k & 1 else hx), (-hy if k & 2 else hy), (zt if k & 4 else z)
        cx = x + lx * c - ly * s
        cy = y + lx * s + ly * c
        r = [M[:, 4 * a] * cx + M[:, 4 * a + 1] * cy + M[:, 4 * a + 2] * cz + M[:, 4 * a + 3] for a in range(3)]
        us.append(r[0] / r[2])
        vs.append(r[1] / r[2])
    U, V = torch.stack(us, 1), torch.stack(vs, 1)
    fin = torch.isfinite(U).all(1) & torch.isfinite(V).all(1)
    raw = torch.stack([U.min(1)[0], V.min(1)[0], U.max(1)[0], V.max(1)[0]], 1)
    raw = torch.where(fin[:, None], raw, torch.full_like(raw, math.nan))
    lim = torch.stack([W, H, W, H], 1)
    clip = torch.where(fin[:, None], torch.minimum(raw.clamp(min=0.0), lim), torch.zeros_like(raw))
    out["raw"][:m], out["clip"][:m] = raw, clip
    out["valid"][:m] = (fin & (raw[:, 0] < W) & (raw[:, 1] < H) & (raw[:, 2] > 0) & (raw[:, 3] > 0)
                        & (x > rng[0]) & (y > rng[1]) & (z > rng[2]) & (x < rng[3]) & (y < rng[4]) & (z < rng[5]))
    out["alpha"][:m] = torch.atan2(y.double(), x.double()) - yaw.double() - math.pi / 2
    out["height"][:m] = clip[:, 3] - clip[:, 1]
    return out


def project_boxes(boxes: torch.Tensor, off, mats: torch.Tensor, img_hw: torch.Tensor, pcd_limit_range=PCD_LIMIT_RANGE):
    """LiDAR boxes [n, 7+] of F ragged frames (off [F + 1] host integers; rows past off[F] belong to no frame and
    get zeros) through each frame's lidar2img (mats [F, 3|4, 4] or [F, 12]; the first three rows are used) into its
    (h, w) image (img_hw [F, 2]). -> dict(raw [n, 4], clip [n, 4], valid [n] bool, alpha [n] float64, height [n]) as
    DESIGN.md "Calibration" defines them."""
    off = _host_offsets(off)
    F = len(off) - 1
    boxes = boxes.reshape(-1, boxes.shape[-1])[:, :7].float().contiguous()
    dev = boxes.device
    n = boxes.shape[0]
    if off[-1] > n:
        raise ValueError("the offsets end past the number of boxes")
    maxn = max((b - a for a, b in zip(off, off[1:])), default=0)
    mats = torch.as_tensor(mats, dtype=torch.float32).reshape(F, -1)[:, :12].contiguous().to(dev)
    img_hw = torch.as_tensor(img_hw).reshape(F, 2).to(device=dev, dtype=torch.float32).contiguous()
    rng = [float(np.float32(v)) for v in pcd_limit_range]
    if len(rng) != 6:
        raise ValueError("pcd_limit_range has six numbers")
    if not boxes.is_cuda:
        return _project_cpu(boxes, off, mats, img_hw, rng)
    raw, clip = (torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(2))
    alpha = torch.empty(n, dtype=torch.float64, device=dev)
    height = torch.empty(n, dtype=torch.float32, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    d_off = torch.tensor(off, dtype=torch.int32, device=dev)
    _ffi.check(_ffi.load().rpc_kitti_project(_ffi.ptr(boxes), n, _ffi.ptr(d_off), F, maxn, _ffi.ptr(mats),
                                             _ffi.ptr(img_hw), _ffi.float_arr(rng), _ffi.ptr(raw), _ffi.ptr(clip),
                                             _ffi.ptr(valid), _ffi.ptr(alpha), _ffi.ptr(height),
                                             _ffi.stream_of(boxes)), "rpc_kitti_project")
    return dict(raw=raw, clip=clip, valid=valid.bool(), alpha=alpha, height=height)


def _inter_2d(d, g):
    """[nd, 4], [ng, 4] -> intersection areas [nd, ng] (0 unless both sides are > 0)."""
    iw = torch.minimum(d[:, None, 2], g[None, :, 2]) - torch.maximum(d[:, None, 0], g[None, :, 0])
    ih = torch.minimum(d[:, None, 3], g[None, :, 3]) - torch.maximum(d[:, None, 1], g[None, :, 1])
    return torch.where((iw > 0) & (ih > 0), iw * ih, torch.zeros_like(iw))


def _overlaps_2d(det, det_off, gt, gt_off, ov_off, maxd, maxg, dev_off=None):
    """2D IoU of every frame's [nd, ng] pairs, flat in the layout of `_overlaps`."""
    total = ov_off[-1]
    if not det.is_cuda:
        parts = []
        for f in range(len(det_off) - 1):
            d, g = det[det_off[f]:det_off[f + 1]], gt[gt_off[f]:gt_off[f + 1]]
            if not (d.shape[0] and g.shape[0]):
                continue
            inter = _inter_2d(d, g)
            wd, hd, wg, hg = d[:, 2] - d[:, 0], d[:, 3] - d[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
            ok = ((wd > 0) & (hd > 0))[:, None] & ((wg > 0) & (hg > 0))[None, :] & (inter > 0)
            union = ((wg * hg)[None, :] + (wd * hd)[:, None]) - inter
            parts.append(torch.where(ok, inter / union, torch.zeros_like(inter)).reshape(-1))
        return torch.cat(parts) if parts else torch.zeros(total, dtype=torch.float32)
    ov = torch.empty(total, dtype=torch.float32, device=det.device)
    d_off, g_off, o_off = dev_off
    _ffi.check(_ffi.load().rpc_kitti_overlaps_2d(
        _ffi.ptr(det), _ffi.ptr(d_off), _ffi.ptr(gt), _ffi.ptr(g_off), _ffi.ptr(o_off), len(det_off) - 1, maxd, maxg,
        0, _ffi.ptr(ov), None, 0, det.shape[0], None, _ffi.stream_of(det)), "rpc_kitti_overlaps_2d")
    return ov


def _stuff_bits(det, det_off, dc, dc_off, maxd, min_ov_cls):
    """-> [C, n_det] uint8: detection j lies in a DontCare region for class c's minimum overlap."""
    C, n = min_ov_cls.numel(), det.shape[0]
    maxc = max((b - a for a, b in zip(dc_off, dc_off[1:])), default=0)
    if maxc > _ffi.KITTI_MAX_DC:
        raise ValueError(f"a frame has {maxc} DontCare boxes; the evaluator takes at most {_ffi.KITTI_MAX_DC}")
    if not det.is_cuda:
        out = torch.zeros((C, n), dtype=torch.uint8)
        for f in range(len(det_off) - 1):
            d, g = det[det_off[f]:det_off[f + 1]], dc[dc_off[f]:dc_off[f + 1]]
            if not (d.shape[0] and g.shape[0]):
                continue
            wd, hd = d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
            ok = (wd > 0) & (hd > 0)
            ratio = torch.where(ok[:, None], _inter_2d(d, g) / (wd * hd)[:, None], torch.zeros(1)).max(1)[0]
            out[:, det_off[f]:det_off[f + 1]] = (ratio[None, :] > min_ov_cls[:, None]).to(torch.uint8)
        return out
    dev = det.device
    out = torch.empty((C, n), dtype=torch.uint8, device=dev)
    d_off = torch.tensor(det_off, dtype=torch.int32, device=dev)
    c_off = torch.tensor(dc_off, dtype=torch.int32, device=dev)
    _ffi.check(_ffi.load().rpc_kitti_overlaps_2d(
        _ffi.ptr(det), _ffi.ptr(d_off), _ffi.ptr(dc), _ffi.ptr(c_off), None, len(det_off) - 1, maxd, maxc, 1, None,
        _ffi.ptr(min_ov_cls), C, n, _ffi.ptr(out), _ffi.stream_of(det)), "rpc_kitti_overlaps_2d")
    return out


def box_overlaps_2d(dets: torch.Tensor, det_off, others: torch.Tensor, other_off, mode: int = 0, min_overlaps=None):
    """2D boxes (x1, y1, x2, y2) of F ragged frames. mode 0: -> (ov, ov_off), the IoU without a +1 of every frame's
    [Nd, Ng] pairs in the layout of `box_overlaps`; exactly 0 when either box has a non-positive side. mode 1:
    others are DontCare boxes (at most KITTI_MAX_DC a frame); -> stuff [C, n_det] uint8 for the C values of
    min_overlaps: some DontCare box of the detection's frame covers more than that share of the detection."""
    if mode not in (0, 1):
        raise ValueError("mode is 0 (IoU) or 1 (DontCare)")
    det_off, other_off = _host_offsets(det_off), _host_offsets(other_off)
    if len(det_off) != len(other_off):
        raise ValueError("the offsets describe different numbers of frames")
    dets = dets.reshape(-1, 4).float().contiguous()
    others = others.reshape(-1, 4).float().contiguous().to(dets.device)
    if det_off[-1] != dets.shape[0] or other_off[-1] != others.shape[0]:
        raise ValueError("the offsets do not end at the number of boxes")
    if mode == 1:
        maxd = max((b - a for a, b in zip(det_off, det_off[1:])), default=0)
        if maxd > _ffi.KITTI_MAX_DET:
            raise ValueError(f"a frame has {maxd} detections; the evaluator takes at most {_ffi.KITTI_MAX_DET}")
        mo = torch.as_tensor(min_overlaps, dtype=torch.float32).reshape(-1).to(dets.device)
        return _stuff_bits(dets, det_off, others, other_off, maxd, mo)
    maxd, maxg = _check_caps(det_off, other_off)
    ov_off = _offsets([(det_off[f + 1] - det_off[f]) * (other_off[f + 1] - other_off[f])
                       for f in range(len(det_off) - 1)])
    dev_off = _device_offsets(det_off, other_off, ov_off, dets.device) if dets.is_cuda else None
    return _overlaps_2d(dets, det_off, others, other_off, ov_off, maxd, maxg, dev_off), ov_off


# ----------------------------------------------------------------------------------- thresholds
def threshold_indices(n_scores: int, n_valid_gt: int) -> list:
    """get_thresholds: the positions, in the descending list of a group's n_scores true-positive scores, of the
    at most 41 recall thresholds (float64 arithmetic, as upstream). The positions depend on the two counts
    only. The skip condition is monotone in the position (true, then false), so each threshold is found by a
    jump to its estimate and a short walk instead of a pass over all scores."""
    n = n_valid_gt
    if n_scores <= 0 or n <= 0:
        return []
    last = n_scores - 1

    def skip(i, cur):
        l = (i + 1) / n
        r = (i + 2) / n if i < last else l
        return (r - cur) < (cur - l) and i < last

    out, cur, start = [], 0.0, 0
    while start <= last and len(out) < N_THR:
        i = min(max(start, int(cur * n - 1.5) - 2), last)
        while i > start and not skip(i - 1, cur):
            i -= 1
        while skip(i, cur):
            i += 1
        out.append(i)
        cur += 1 / 40.0
        start = i + 1
    return out


# ----------------------------------------------------------------------------------- the metric
def _field(d, names, default=None):
    for n in names:
        if isinstance(d, dict) and n in d and d[n] is not None:
            return d[n]
    return default


class KittiAP:
    """KITTI BEV / 3D average precision over the frames given to `update`.

    class_names: the detector's classes, label k <-> class_names[k]. min_overlaps: {name: (strict, loose)}
    for classes outside the KITTI table (Car 0.7 / 0.5, Pedestrian and Cyclist 0.5 / 0.25) or to override it.
    `compute()` -> {"KITTI/{Class}_{BEV|3D}_AP{11|40}_{easy|moderate|hard}_{strict|loose}": float, ...,
    "KITTI/Overall_{BEV|3D}_AP{11|40}_{difficulty}": mean over the classes of the strict values}. The
    accumulator (the frames' tensors) stays on the detections' device.

    metrics: any subset of ("BEV", "3D", "2D", "AOS"), reported in that order; "2D" is the image-plane `bbox`
    metric (the class's strict minimum overlap in both tables, DontCare regions honoured), "AOS" the orientation
    similarity on the 2D matching. Both need every frame's 2D boxes: a `lidar2img` in the ground-truth dict, or a
    `bbox` on both sides. pcd_limit_range: detections of a calibrated frame whose bottom centre is not strictly
    inside it are removed, like those that project outside the image."""

    def __init__(self, class_names, min_overlaps=None, metrics=METRICS, pcd_limit_range=PCD_LIMIT_RANGE):
        self.class_names = list(class_names)
        if not self.class_names:
            raise ValueError("KittiAP needs at least one class name")
        metrics = [metrics] if isinstance(metrics, str) else list(metrics)
        bad = [m for m in metrics if m not in ALL_METRICS]
        if bad or not metrics:
            raise ValueError(f"metrics is a non-empty subset of {ALL_METRICS}, got {metrics}")
        self.metrics = tuple(m for m in ALL_METRICS if m in metrics)
        self.pcd_limit_range = tuple(float(v) for v in pcd_limit_range)
        if len(self.pcd_limit_range) != 6:
            raise ValueError("pcd_limit_range has six numbers")
        mo = dict(min_overlaps or {})
        self.min_overlaps = []
        for n in self.class_names:
            if n in mo:
                s, l = mo[n]
            elif n in MIN_OVERLAP_STRICT:
                s, l = MIN_OVERLAP_STRICT[n], MIN_OVERLAP_LOOSE[n]
            else:
                raise ValueError(f"class {n!r} is not in the KITTI overlap table: pass min_overlaps={{{n!r}: "
                                 "(strict, loose)}")
            self.min_overlaps.append((float(s), float(l)))
        self.reset()

    def reset(self):
        self._det, self._gt = [], []     # one tuple of concatenated tensors per update() call
        self._nd, self._ng = [], []      # detections / ground truths of every frame
        self._cal = []                   # per update() call: the calibration side (see _calib_fields)
        self._ndc, self._has = [], []    # DontCare boxes of every frame; whether it has a lidar2img
        self._device = None

    def __len__(self):
        return len(self._nd)

    def update(self, preds, gts):
        """preds: the per-frame dicts of `predict` (bboxes_3d [n, 7+], scores_3d, labels_3d; optional
        bbox_height, the 2D box height in pixels). gts: per frame a dict with bboxes_3d [m, 7+] and labels_3d
        (int64; -1: any other class) and optionally neighbor (int64: the class this object is the neighbour
        class of — Van for Car, Person_sitting for Pedestrian — or -1), bbox_height, occluded, truncated; or a
        (boxes, labels) pair. Missing fields: height +inf, occluded 0, truncated 0, no neighbour.

        Calibration (mmdet3d's meta names, in the ground-truth dict): lidar2img [3|4, 4], img_shape (h, w), bbox
        [m, 4] annotated 2D boxes, alpha [m], dontcare [k, 4] 2D boxes. A frame with lidar2img has its detections
        projected: the invalid ones are removed and the projected box's height overrides bbox_height. A
        prediction may carry bbox [n, 4] (and alpha [n]) for a frame without lidar2img."""
        if len(preds) != len(gts):
            raise ValueError(f"{len(preds)} frames of detections, {len(gts)} of ground truth")
        dets, truths, cals = [], [], []
        for p, g in zip(preds, gts):
            box = p["bboxes_3d"]
            box = getattr(box, "tensor", box)
            if self._device is None:
                self._device = box.device     # the accumulator lives where the first detections do
            n = box.shape[0]
            if n > _ffi.KITTI_MAX_DET:
                raise ValueError(f"a frame has {n} detections; the evaluator takes at most {_ffi.KITTI_MAX_DET}")
            f32 = dict(dtype=torch.float32, device=self._device)
            h = p.get("bbox_height")
            dets.append((box.detach().reshape(n, box.shape[-1])[:, :7].to(**f32),
                         p["scores_3d"].detach().reshape(n).to(**f32),
                         p["labels_3d"].detach().reshape(n).to(device=self._device, dtype=torch.int64),
                         torch.full((n,), math.inf, **f32) if h is None else torch.as_tensor(h).reshape(n).to(**f32)))
            if isinstance(g, (tuple, list)):
                g = dict(bboxes_3d=g[0], labels_3d=g[1])
            gb = _field(g, ("bboxes_3d", "gt_bboxes_3d", "boxes"))
            gb = torch.as_tensor(getattr(gb, "tensor", gb))
            m = gb.shape[0]
            if m > _ffi.KITTI_MAX_GT:
                raise ValueError(f"a frame has {m} ground truths; the evaluator takes at most {_ffi.KITTI_MAX_GT}")
            i64 = dict(dtype=torch.int64, device=self._device)

            def opt(names, fill, kw):
                v = _field(g, names)
                return torch.full((m,), fill, **kw) if v is None else torch.as_tensor(v).reshape(m).to(**kw)

            truths.append((gb.detach().reshape(m, gb.shape[-1])[:, :7].to(**f32),
                           torch.as_tensor(_field(g, ("labels_3d", "gt_labels_3d", "labels"))).reshape(m).to(**i64),
                           opt(("neighbor",), -1, i64), opt(("bbox_height",), math.inf, f32),
                           opt(("occluded",), 0, f32), opt(("truncated",), 0, f32)))
            cals.append(self._calib_fields(p, g, n, m, f32))
        if dets:   # nothing is kept of a call that raised
            self._nd += [d[0].shape[0] for d in dets]
            self._ng += [t[0].shape[0] for t in truths]
            self._det.append(tuple(torch.cat([d[k] for d in dets]) for k in range(4)))
            self._gt.append(tuple(torch.cat([t[k] for t in truths]) for k in range(6)))
            self._ndc += [c[7].shape[0] for c in cals]
            self._has += [c[8] for c in cals]
            self._cal.append(tuple(torch.cat([c[k] for c in cals]) for k in range(8)))

    def _calib_fields(self, p, g, n, m, f32):
        """One frame's calibration side -> (mat [1, 12], hw [1, 2], det bbox [n, 4], det alpha [n], gt bbox [m, 4],
        gt alpha [m] — NaN where not given —, gt height given [m] bool, dontcare [k, 4], has lidar2img)."""
        nan = math.nan
        l2i = _field(g, ("lidar2img",))
        shape = _field(g, ("img_shape",))
        has = l2i is not None
        if has and shape is None:
            raise ValueError("a frame with lidar2img needs img_shape (h, w)")

        def given(d, name, rows, cols):
            v = _field(d, (name,))
            size = (rows, cols) if cols else (rows,)
            kw = f32 if cols else dict(dtype=torch.float64, device=self._device)    # the angles are float64
            return torch.full(size, nan, **kw) if v is None else torch.as_tensor(v).detach().reshape(size).to(**kw)

        det_bbox, gt_bbox = given(p, "bbox", n, 4), given(g, "bbox", m, 4)
        if ("2D" in self.metrics or "AOS" in self.metrics) and not has and (
                _field(p, ("bbox",)) is None or _field(g, ("bbox",)) is None):
            raise ValueError("the 2D and AOS metrics need every frame's 2D boxes: lidar2img (and img_shape) in the "
                             "ground-truth dict, or bbox in both the prediction and the ground truth")
        mat = (torch.as_tensor(l2i).detach().to(**f32).reshape(-1)[:12] if has else torch.zeros(12, **f32)).reshape(1, 12)
        if mat.shape[1] != 12:
            raise ValueError("lidar2img is a [3, 4] or [4, 4] matrix")
        hw = torch.tensor([float(shape[0]), float(shape[1])] if has else [0.0, 0.0], **f32).reshape(1, 2)
        dc = _field(g, ("dontcare",))
        dc = torch.zeros((0, 4), **f32) if dc is None else torch.as_tensor(dc).detach().reshape(-1, 4).to(**f32)
        if dc.shape[0] > _ffi.KITTI_MAX_DC:
            raise ValueError(f"a frame has {dc.shape[0]} DontCare boxes; the evaluator takes at most {_ffi.KITTI_MAX_DC}")
        hgiven = torch.full((m,), _field(g, ("bbox_height",)) is not None, dtype=torch.bool, device=self._device)
        return (mat, hw, det_bbox, given(p, "alpha", n, 0), gt_bbox, given(g, "alpha", m, 0), hgiven,
                dc, has)

    # ------------------------------------------------------------------ pieces (the tests call them)
    def _flags(self, dl, dh, gl, gn, gh, go, gt_, valid=None):
        """flag_det [C * 3, n_det], flag_gt [C * 3, n_gt] int8; row c * 3 + d. valid [n_det] bool: a detection
        the calibration removed has flag -1 in every row, which no pass can tell from its absence."""
        fd, fg = [], []
        one, zero, neg = (torch.tensor(v, dtype=torch.int8, device=dl.device) for v in (1, 0, -1))
        for c in range(len(self.class_names)):
            for d in range(3):
                vc = torch.where(gl == c, one, torch.where(gn == c, zero, neg))
                ign = (go > MAX_OCCLUSION[d]) | (gt_ > MAX_TRUNCATION[d]) | (gh <= MIN_HEIGHT[d])
                fg.append(torch.where((vc == 1) & ~ign, zero, torch.where((vc == 0) | (ign & (vc == 1)), one, neg)))
                fd.append(torch.where(dh < MIN_HEIGHT[d], one, torch.where(dl == c, zero, neg)))
        fd = torch.stack(fd)
        if valid is not None:
            fd = torch.where(valid[None, :], fd, neg)
        return fd.contiguous(), torch.stack(fg).contiguous()

    def _min_ov(self, dev):
        """[C * 3 * 2] fp32; group (c * 3 + d) * 2 + table."""
        return torch.tensor([self.min_overlaps[c][t] for c in range(len(self.class_names)) for _ in range(3)
                             for t in range(2)], dtype=torch.float32, device=dev)

    def compute(self) -> dict:
        C = len(self.class_names)
        G = C * 3 * 2
        fams = self._families()
        res = {m: ([0.0] * G, [0.0] * G) for m in self.metrics}
        if self._nd:
            detail = {}
            counts, nthr = self._counts(detail=detail)
            ap11, ap40 = _average_precision(counts, nthr)
            for k, fam in enumerate(fams):
                if fam in self.metrics:
                    res[fam] = (ap11[k * G:(k + 1) * G], ap40[k * G:(k + 1) * G])
            if "AOS" in self.metrics:
                k = fams.index("2D")
                res["AOS"] = _average_precision(counts[k * G:(k + 1) * G], nthr[k * G:(k + 1) * G],
                                                detail["sim"].double() / SIM_ONE)
        keys = [(c, d, t) for c in range(C) for d in range(3) for t in range(2)]
        out = {}
        for m in self.metrics:
            for (c, d, t), a11, a40 in zip(keys, *res[m]):
                for name, v in (("AP11", a11), ("AP40", a40)):
                    out[f"KITTI/{self.class_names[c]}_{m}_{name}_{DIFFICULTIES[d]}_{TABLES[t]}"] = float(v)
        for m in self.metrics:
            for name in ("AP11", "AP40"):
                for d in range(3):
                    vals = [out[f"KITTI/{n}_{m}_{name}_{DIFFICULTIES[d]}_strict"] for n in self.class_names]
                    out[f"KITTI/Overall_{m}_{name}_{DIFFICULTIES[d]}"] = float(sum(vals) / len(vals))
        return out

    def _families(self):
        """The matchings the metrics need, in the order of ALL_METRICS: AOS rides on the 2D matching."""
        need = set(self.metrics) | ({"2D"} if "AOS" in self.metrics else set())
        return [m for m in ("BEV", "3D", "2D") if m in need]

    def _calibrate(self, det, dh, gt, gh, det_off, gt_off):
        """The calibration side of all frames -> dict(valid [n_det] bool, det_height, gt_height, det_box / gt_box
        [., 4], det_alpha / gt_alpha, dc [k, 4], dc_off). Frames without lidar2img keep what they were given."""
        dev = self._device
        mat, hw, dbox_in, dalpha_in, gbox_in, galpha_in, hgiven, dc = (
            torch.cat([c[k] for c in self._cal]).contiguous() for k in range(8))
        has = torch.tensor(self._has, dtype=torch.bool, device=dev)
        out = {}
        for side, box, off, box_in, alpha_in in (("det", det, det_off, dbox_in, dalpha_in),
                                                 ("gt", gt, gt_off, gbox_in, galpha_in)):
            pr = project_boxes(box, off, mat, hw, self.pcd_limit_range)
            cal = has[_frame_index(off, dev)]
            out[side + "_cal"], out[side + "_proj"] = cal, pr
            given = ~torch.isnan(box_in).any(-1)
            if side == "det":    # a calibrated frame's detections take the projection; its ground truth the annotation
                out["valid"] = pr["valid"] | ~cal
                out["det_box"] = torch.where(cal[:, None], pr["clip"], box_in).contiguous()
                out["det_height"] = torch.where(cal, pr["height"], dh)
            else:
                nan = torch.full_like(box_in, math.nan)
                out["gt_box"] = torch.where(given[:, None], box_in, torch.where(cal[:, None], pr["clip"], nan)).contiguous()
                b = out["gt_box"]
                inf = torch.full_like(gh, math.inf)
                out["gt_height"] = torch.where(hgiven, gh, torch.where(given | cal, b[:, 3] - b[:, 1], inf))
            out[side + "_alpha"] = torch.where(torch.isnan(alpha_in), pr["alpha"], alpha_in).contiguous()
        out["dc"], out["dc_off"] = dc, _offsets(self._ndc)
        return out

    def _counts(self, overlaps=None, detail=None):
        """-> counts [K * G, 41, 3] int64 (tp, fp, fn; CPU) and nthr [K * G] (list); family-major groups, the K
        families of `_families()` (BEV and 3D by default). overlaps: one flat overlap tensor per family to use
        instead of the computed ones; detail: a dict that receives the intermediate results (overlaps, pass-1
        scores, thresholds, the similarity sums [G, 41] int64 in units of 1 / SIM_ONE, the calibration side)."""
        dev = self._device
        fams = self._families()
        K = len(fams)
        det_off, gt_off = _offsets(self._nd), _offsets(self._ng)
        F = len(self._nd)
        maxd, maxg = _check_caps(det_off, gt_off)
        ov_off = _offsets([(det_off[f + 1] - det_off[f]) * (gt_off[f + 1] - gt_off[f]) for f in range(F)])
        det, score, dl, dh = (torch.cat([d[k] for d in self._det]).contiguous() for k in range(4))
        gt, gl, gn, gh, go, gtr = (torch.cat([g[k] for g in self._gt]).contiguous() for k in range(6))
        cal = None
        if any(self._has) or "2D" in fams:
            cal = self._calibrate(det, dh, gt, gh, det_off, gt_off)
            dh, gh = cal["det_height"], cal["gt_height"]
        fdet, fgt = self._flags(dl, dh, gl, gn, gh, go, gtr, None if cal is None else cal["valid"])
        min_ov = self._min_ov(dev)
        G = min_ov.numel()
        # the 2D and AOS metrics take the class's strict value in both tables
        min_ov_2d = min_ov.view(-1, 2)[:, :1].expand(-1, 2).reshape(-1).contiguous()
        n_det, n_gt = det_off[-1], gt_off[-1]
        cuda = det.is_cuda
        dev_off = _device_offsets(det_off, gt_off, ov_off, dev) if cuda else None
        if overlaps is None:
            overlaps = [_overlaps_2d(cal["det_box"], det_off, cal["gt_box"], gt_off, ov_off, maxd, maxg, dev_off)
                        if m == "2D" else _overlaps(det, det_off, gt, gt_off, ov_off, maxd, maxg, METRICS.index(m), dev_off)
                        for m in fams]
        overlaps = list(overlaps)
        if len(overlaps) != K:
            raise ValueError(f"{K} overlap tensors are needed ({fams}), {len(overlaps)} given")
        mins = [min_ov_2d if m == "2D" else min_ov for m in fams]
        frame = (det_off, gt_off, ov_off, maxd, maxg, dev_off)
        # pass 1: the true-positive scores of every group, all families
        tps = torch.stack([_match_scores(ov, frame, score, fdet, fgt, mo) for ov, mo in zip(overlaps, mins)])  # [K, G, n_gt]
        srt = tps.sort(dim=-1, descending=True)[0]
        nemit = (tps > NO).sum(-1).reshape(-1)
        nvalid = (fgt == 0).sum(-1)
        host = torch.cat([nemit, nvalid]).cpu().tolist()            # the one host read between the passes
        nemit, nvalid = host[:K * G], host[K * G:]
        idx = [threshold_indices(nemit[q], nvalid[(q % G) // 2]) for q in range(K * G)]
        nthr = [len(v) for v in idx]
        pad = torch.tensor([v + [0] * (N_THR - len(v)) for v in idx], dtype=torch.int64, device=dev).view(K, G, N_THR)
        if n_gt:
            thr = srt.gather(-1, pad).contiguous()
        else:
            thr = torch.zeros((K, G, N_THR), dtype=torch.float32, device=dev)
        nthr_t = torch.tensor(nthr, dtype=torch.int32, device=dev).view(K, G)
        # pass 2: tp / fp / fn at every threshold; the 2D family also the DontCare bits and the similarity sums
        counts, sim, stuff = [], torch.zeros((G, N_THR), dtype=torch.int64, device=dev), None
        for k, (m, ov) in enumerate(zip(fams, overlaps)):
            if m != "2D":
                counts.append(_match_counts(ov, frame, score, fdet, fgt, mins[k], thr[k], nthr_t[k]))
                continue
            if cal["dc"].shape[0]:
                stuff = _stuff_bits(cal["det_box"], det_off, cal["dc"], cal["dc_off"], maxd,
                                    min_ov.view(-1, 6)[:, 0].contiguous())
            alpha = (cal["det_alpha"], cal["gt_alpha"]) if "AOS" in self.metrics else None
            c2, sim = _match_counts(ov, frame, score, fdet, fgt, mins[k], thr[k], nthr_t[k], stuff=stuff, alpha=alpha,
                                    ext=True)
            counts.append(c2)
        counts = torch.stack(counts).reshape(K * G, N_THR, 3)
        # the one host read at the end: the counts and the similarity sums together
        host = torch.cat([counts.reshape(-1).to(torch.int64), sim.reshape(-1)]).cpu()
        counts, sim = host[:K * G * N_THR * 3].view(K * G, N_THR, 3), host[K * G * N_THR * 3:].view(G, N_THR)
        if detail is not None:
            detail.update(overlaps=overlaps, ov_off=ov_off, det_off=det_off, gt_off=gt_off, tp_scores=tps, thr=thr,
                          nthr=nthr, flag_det=fdet, flag_gt=fgt, min_ov=min_ov, score=score, n_valid_gt=nvalid,
                          families=fams, sim=sim, stuff=stuff, calib=cal)
        return counts, nthr


def _match_scores(ov, frame, score, fdet, fgt, min_ov):
    """Matcher pass 1 -> tp_score [G, n_gt] fp32 (NO where the ground truth has no true positive)."""
    det_off, gt_off, ov_off, maxd, maxg, dev_off = frame
    G = min_ov.numel()
    ntab = G // fdet.shape[0]
    n_det, n_gt = det_off[-1], gt_off[-1]
    if not score.is_cuda:
        out = torch.full((G, n_gt), NO, dtype=torch.float32)
        sl, mo = score.tolist(), min_ov.tolist()
        for g in range(G):
            fr, gr = fdet[g // ntab].tolist(), fgt[g // ntab].tolist()
            for o, s, fd, fg, g0 in _frames_cpu(ov, ov_off, det_off, gt_off, sl, fr, gr):
                for i, v in _match_frame(o, s, fd, fg, mo[g], 0.0, False)[3].items():
                    out[g, g0 + i] = v
        return out
    out = torch.empty((G, n_gt), dtype=torch.float32, device=score.device)
    d_off, g_off, o_off = dev_off
    _ffi.check(_ffi.load().rpc_kitti_match_scores(
        _ffi.ptr(ov), _ffi.ptr(o_off), _ffi.ptr(d_off), _ffi.ptr(g_off), len(det_off) - 1, maxd, maxg,
        _ffi.ptr(score), _ffi.ptr(fdet), _ffi.ptr(fgt), n_det, n_gt, _ffi.ptr(min_ov), G, ntab, _ffi.ptr(out),
        _ffi.stream_of(score)), "rpc_kitti_match_scores")
    return out


def _match_counts(ov, frame, score, fdet, fgt, min_ov, thr, nthr, stuff=None, alpha=None, ext=False):
    """Matcher pass 2 -> counts [G, 41, 3] int32 (tp, fp, fn) summed over the frames. ext (the 2D family):
    stuff [G / gps, n_det] uint8 or None, alpha = (per detection, per ground truth) or None; then -> (counts, sim
    [G, 41] int64, the similarity sums in units of 1 / SIM_ONE), through rpc_kitti_match_counts_aos."""
    det_off, gt_off, ov_off, maxd, maxg, dev_off = frame
    G = min_ov.numel()
    ntab = G // fdet.shape[0]
    gps = G // stuff.shape[0] if stuff is not None else 1
    n_det, n_gt = det_off[-1], gt_off[-1]
    if not score.is_cuda:
        out = torch.zeros((G, N_THR, 3), dtype=torch.int32)
        sim = torch.zeros((G, N_THR), dtype=torch.int64)
        sl, mo, tl, nl = score.tolist(), min_ov.tolist(), thr.tolist(), nthr.tolist()
        al = None if alpha is None else (alpha[0].tolist(), alpha[1].tolist())
        for g in range(G):
            if not nl[g]:
                continue
            fr, gr = fdet[g // ntab].tolist(), fgt[g // ntab].tolist()
            st = None if stuff is None else stuff[g // gps].tolist()
            for f, (o, s, fd, fg, _) in enumerate(_frames_cpu(ov, ov_off, det_off, gt_off, sl, fr, gr)):
                d0, d1, g0, g1 = det_off[f], det_off[f + 1], gt_off[f], gt_off[f + 1]
                fa = None if al is None else (al[0][d0:d1], al[1][g0:g1])
                for k in range(nl[g]):
                    sims = []
                    tp, fp, fn, _e = _match_frame(o, s, fd, fg, mo[g], tl[g][k], True,
                                                  None if st is None else st[d0:d1], fa, sims)
                    out[g, k, 0] += tp
                    out[g, k, 1] += fp
                    out[g, k, 2] += fn
                    sim[g, k] += sum(sims)
        return (out, sim) if ext else out
    out = torch.empty((G, N_THR, 3), dtype=torch.int32, device=score.device)
    thr, nthr = thr.contiguous(), nthr.contiguous()
    d_off, g_off, o_off = dev_off
    head = (_ffi.ptr(ov), _ffi.ptr(o_off), _ffi.ptr(d_off), _ffi.ptr(g_off), len(det_off) - 1, maxd, maxg,
            _ffi.ptr(score), _ffi.ptr(fdet), _ffi.ptr(fgt), n_det, n_gt, _ffi.ptr(min_ov), G, ntab, _ffi.ptr(thr),
            _ffi.ptr(nthr))
    if not ext:
        _ffi.check(_ffi.load().rpc_kitti_match_counts(*head, _ffi.ptr(out), _ffi.stream_of(score)),
                   "rpc_kitti_match_counts")
        return out
    sim = torch.empty((G, N_THR), dtype=torch.int64, device=score.device)
    ad, ag = (None, None) if alpha is None else (alpha[0].contiguous(), alpha[1].contiguous())
    _ffi.check(_ffi.load().rpc_kitti_match_counts_aos(*head, _ffi.ptr(stuff), gps, _ffi.ptr(ad), _ffi.ptr(ag),
                                                      _ffi.ptr(out), _ffi.ptr(sim), _ffi.stream_of(score)),
               "rpc_kitti_match_counts_aos")
    return out, sim


def _average_precision(counts, nthr, sim=None):
    """counts [Q, 41, 3] int64 (CPU), nthr [Q] -> (AP11 [Q], AP40 [Q]) lists of floats. precision[k] =
    tp / (tp + fp) at threshold k (0 beyond the group's thresholds, and where nothing was detected), then the
    running maximum from the right; AP11 = 100 * sum(precision[0::4]) / 11, AP40 = 100 * sum(precision[1:]) / 40.
    sim [Q, 41] float64: the orientation similarity sums, which replace tp in the numerator (AOS)."""
    c = counts.double()
    tp, fp = c[..., 0], c[..., 1]
    live = torch.arange(N_THR)[None, :] < torch.tensor(nthr)[:, None]
    num = tp if sim is None else sim.double()
    prec = torch.where(live & (tp + fp > 0), num / (tp + fp).clamp(min=1), torch.zeros_like(tp))
    prec = prec.flip(-1).cummax(-1)[0].flip(-1)
    ap11 = (100.0 * prec[:, 0::4].sum(-1) / 11.0).tolist()
    ap40 = (100.0 * prec[:, 1:].sum(-1) / 40.0).tolist()
    return ap11, ap40
