"""nuScenes detection score (mAP, the five true-positive errors, NDS) from the per-frame dicts `predict` returns.

Restates nuscenes-devkit `eval/detection` (`accumulate`, `calc_ap`, `calc_tp`, `detection_cvpr_2019`) in the LiDAR
frame; the specification is written out in DESIGN.md "nuScenes detection score". Boxes are LiDAR boxes (x, y, z,
dx, dy, dz, yaw, vx, vy) as AdversarialCenterPoint's `predict` returns them; 7-column boxes count as velocity 0.
The bike-rack filter, pose transforms beyond a per-frame `ego_origin` and the json submission format are not part
of it.

CUDA tensors: sorting, the filtering flags and the attribute rule are torch, then the HIP kernels of
csrc/nuscenes_eval.hip — `rpc_nus_match` (the greedy matcher for all frames x classes x thresholds in one launch)
and `rpc_nus_tp_errors` — then ONE host read (matches, errors, scores, labels, flags together) and the curves in
float64 on the host. CPU tensors take a plain Python / torch path with the same semantics (slow; it makes the
metric usable and testable without a GPU, like kitti_eval.py's).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _ffi
from .center_head import NUS_TASKS
from .kitti_eval import _field, _host_offsets, _offsets

__all__ = ["NuScenesDetectionScore", "center_matches", "DIST_THS", "DIST_TH_TP", "MIN_RECALL", "MIN_PRECISION",
           "MAX_BOXES_PER_SAMPLE", "CLASS_RANGE", "ATTRIBUTES", "DEFAULT_ATTRIBUTE", "TP_METRICS"]

DIST_THS = (0.5, 1.0, 2.0, 4.0)
DIST_TH_TP = 2.0
MIN_RECALL = 0.1
MIN_PRECISION = 0.1
MAX_BOXES_PER_SAMPLE = 500
CLASS_RANGE = {"car": 50.0, "truck": 50.0, "bus": 50.0, "trailer": 50.0, "construction_vehicle": 50.0,
               "pedestrian": 40.0, "motorcycle": 40.0, "bicycle": 40.0, "traffic_cone": 30.0, "barrier": 30.0}
ATTRIBUTES = ("cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing",
              "pedestrian.sitting_lying_down", "vehicle.moving", "vehicle.parked", "vehicle.stopped")
DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "trailer": "vehicle.parked", "truck": "vehicle.parked",
                     "construction_vehicle": "vehicle.parked", "bus": "vehicle.moving",
                     "pedestrian": "pedestrian.moving", "motorcycle": "cycle.without_rider",
                     "bicycle": "cycle.without_rider", "barrier": None, "traffic_cone": None}
TP_METRICS = ("trans", "scale", "orient", "vel", "attr")
MEAN_NAMES = ("mATE", "mASE", "mAOE", "mAVE", "mAAE")
# errors that are not defined for a class: NaN, and left out of the means
UNDEFINED = {"traffic_cone": ("attr", "vel", "orient"), "barrier": ("attr", "vel")}
MOVING_SPEED = 0.2
_MOVING = {"car": "vehicle.moving", "construction_vehicle": "vehicle.moving", "bus": "vehicle.moving",
           "truck": "vehicle.moving", "trailer": "vehicle.moving", "bicycle": "cycle.with_rider",
           "motorcycle": "cycle.with_rider"}
_STILL = {"pedestrian": "pedestrian.standing", "bus": "vehicle.stopped"}
FIRST_IND = int(round(100 * MIN_RECALL)) + 1   # 11


def _attr_id(name):
    return -1 if name is None else ATTRIBUTES.index(name)


# ----------------------------------------------------------------------------------- the matcher
def _match_cpu(det_xy, det_label, det_keep, det_off, gt_xy, gt_label, gt_keep, gt_off, n_classes, thr):
    """The greedy matcher in Python over fp32 squared distances (one torch expression per frame, every operation
    rounded to fp32 as the kernel's). -> match [n_thr, n_det] int32."""
    n_det = det_off[-1]
    match = torch.full((len(thr), n_det), -1, dtype=torch.int32)
    t2 = (torch.tensor(thr, dtype=torch.float32) * torch.tensor(thr, dtype=torch.float32)).tolist()
    dl, dk, gl, gk = det_label.tolist(), det_keep.tolist(), gt_label.tolist(), gt_keep.tolist()
    for f in range(len(det_off) - 1):
        d0, d1, g0, g1 = det_off[f], det_off[f + 1], gt_off[f], gt_off[f + 1]
        if d1 == d0 or g1 == g0:
            continue
        dx = gt_xy[None, g0:g1, 0] - det_xy[d0:d1, None, 0]
        dy = gt_xy[None, g0:g1, 1] - det_xy[d0:d1, None, 1]
        d2 = (dx * dx + dy * dy).tolist()
        for c in range(n_classes):
            rows = [i for i in range(g1 - g0) if gk[g0 + i] and gl[g0 + i] == c]
            dets = [j for j in range(d1 - d0) if dk[d0 + j] and dl[d0 + j] == c]
            if not rows or not dets:
                continue
            for t, tt in enumerate(t2):
                free = list(rows)
                for j in dets:
                    best, bi = math.inf, -1
                    for i in free:
                        if d2[j][i] < best:
                            best, bi = d2[j][i], i
                    if bi >= 0 and best < tt:
                        free.remove(bi)
                        match[t, d0 + j] = g0 + bi
    return match


def center_matches(det_xy, det_label, det_keep, det_off, gt_xy, gt_label, gt_keep, gt_off, n_classes,
                   thresholds=DIST_THS, _dev_off=None):
    """The greedy centre-distance matcher of F frames in one call. det_xy [sum Nd, 2], gt_xy [sum Ng, 2] centres,
    *_label integer classes, *_keep flags (0: filtered), det_off / gt_off [F + 1] host integers (a device tensor
    is read back); the detections stand in evaluation order inside each frame. -> match [len(thresholds), sum Nd]
    int32 on the detections' device: the global row of the ground truth each detection took, or -1. At most
    NUS_MAX_DET / NUS_MAX_GT boxes per frame and NUS_MAX_THR thresholds (ValueError above)."""
    det_off, gt_off = _host_offsets(det_off), _host_offsets(gt_off)
    if len(det_off) != len(gt_off):
        raise ValueError("det_off and gt_off describe different numbers of frames")
    thr = [float(t) for t in thresholds]
    if len(thr) > _ffi.NUS_MAX_THR:
        raise ValueError(f"{len(thr)} thresholds; the matcher takes at most {_ffi.NUS_MAX_THR}")
    dev = det_xy.device
    det_xy = det_xy.reshape(-1, 2).float().contiguous()
    gt_xy = gt_xy.reshape(-1, 2).float().contiguous().to(dev)
    n_det, n_gt = det_xy.shape[0], gt_xy.shape[0]
    if det_off[-1] != n_det or gt_off[-1] != n_gt:
        raise ValueError("the offsets do not end at the number of boxes")
    maxd = max((b - a for a, b in zip(det_off, det_off[1:])), default=0)
    maxg = max((b - a for a, b in zip(gt_off, gt_off[1:])), default=0)
    if maxd > _ffi.NUS_MAX_DET or maxg > _ffi.NUS_MAX_GT:
        raise ValueError(f"a frame has {maxd} detections / {maxg} ground truths; the matcher takes at most "
                         f"{_ffi.NUS_MAX_DET} / {_ffi.NUS_MAX_GT} per frame")
    i32 = dict(dtype=torch.int32, device=dev)
    i8 = dict(dtype=torch.int8, device=dev)
    det_label, gt_label = det_label.reshape(-1).to(**i32).contiguous(), gt_label.reshape(-1).to(**i32).contiguous()
    det_keep, gt_keep = (det_keep.reshape(-1) != 0).to(**i8).contiguous(), (gt_keep.reshape(-1) != 0).to(**i8).contiguous()
    if not det_xy.is_cuda:
        return _match_cpu(det_xy, det_label, det_keep, det_off, gt_xy, gt_label, gt_keep, gt_off, int(n_classes), thr)
    match = torch.empty((len(thr), n_det), **i32)
    d_off, g_off = _dev_off or (torch.tensor(det_off, **i32), torch.tensor(gt_off, **i32))
    thr_t = torch.tensor(thr, dtype=torch.float32, device=dev)
    _ffi.check(_ffi.load().rpc_nus_match(
        _ffi.ptr(det_xy), _ffi.ptr(det_label), _ffi.ptr(det_keep), _ffi.ptr(d_off), _ffi.ptr(gt_xy),
        _ffi.ptr(gt_label), _ffi.ptr(gt_keep), _ffi.ptr(g_off), len(det_off) - 1, maxd, maxg, n_det, n_gt,
        int(n_classes), _ffi.ptr(thr_t), len(thr), _ffi.ptr(match), _ffi.stream_of(det_xy)), "rpc_nus_match")
    return match


# ----------------------------------------------------------------------------------- true-positive errors
def _tp_errors(det, gt, match, period, det_attr, gt_attr):
    """err [n_det, 5] (trans, scale, orient, vel, attr) of detection j against ground truth match[j]; NaN rows
    where match[j] < 0. CUDA: rpc_nus_tp_errors in fp32. CPU: the same expressions in torch float64."""
    n_det, n_gt = det.shape[0], gt.shape[0]
    if det.is_cuda:
        err = torch.empty((n_det, 5), dtype=torch.float32, device=det.device)
        _ffi.check(_ffi.load().rpc_nus_tp_errors(
            _ffi.ptr(det), _ffi.ptr(gt), _ffi.ptr(match), _ffi.ptr(period), _ffi.ptr(det_attr), _ffi.ptr(gt_attr),
            n_det, n_gt, _ffi.ptr(err), _ffi.stream_of(det)), "rpc_nus_tp_errors")
        return err
    err = torch.full((n_det, 5), math.nan, dtype=torch.float64)
    hit = (match >= 0).nonzero().reshape(-1)
    if hit.numel() == 0:
        return err
    d, g = det[hit].double(), gt[match[hit].long()].double()
    p = (2.0 - (period[hit] < 4.0).double()) * math.pi   # pi or 2 pi, in float64 here
    err[hit, 0] = torch.sqrt((g[:, 0] - d[:, 0]) ** 2 + (g[:, 1] - d[:, 1]) ** 2)
    inter = torch.minimum(d[:, 3:6], g[:, 3:6]).prod(-1)
    iou = inter / (g[:, 3:6].prod(-1) + d[:, 3:6].prod(-1) - inter)
    ok = (d[:, 3:6] > 0).all(-1) & (g[:, 3:6] > 0).all(-1)
    err[hit, 1] = torch.where(ok, 1.0 - iou, torch.ones_like(iou))
    v = torch.remainder(g[:, 6] - d[:, 6] + p / 2, p) - p / 2
    err[hit, 2] = torch.where(v > math.pi, v - 2 * math.pi, v).abs()
    err[hit, 3] = torch.sqrt((g[:, 7] - d[:, 7]) ** 2 + (g[:, 8] - d[:, 8]) ** 2)
    ga, da = gt_attr[match[hit].long()], det_attr[hit]
    err[hit, 4] = torch.where(ga < 0, torch.full_like(p, math.nan), (ga != da).double())
    return err


# ----------------------------------------------------------------------------------- curves (host, float64)
def _cummean(x):
    """The NaN-ignoring cumulative mean: 1 everywhere if all values are NaN, 0 where nothing was seen yet."""
    nan = np.isnan(x)
    if nan.all():
        return np.ones(len(x))
    s = np.cumsum(np.where(nan, 0.0, x))
    n = np.cumsum(~nan)
    return np.divide(s, n, out=np.zeros_like(s), where=n != 0)


def _curves(tp, score, npos, errs):
    """One class at one threshold: tp [n] bool, score [n] float64 in evaluation order, npos, errs [n, 5] float64
    or None (only the precision is wanted). -> (precision [101], confidence [101], error curves [5, 101])."""
    if npos == 0 or not tp.any():
        return np.zeros(101), np.zeros(101), np.ones((5, 101))
    ctp = np.cumsum(tp).astype(np.float64)
    cfp = np.cumsum(~tp).astype(np.float64)
    prec, rec = ctp / (ctp + cfp), ctp / float(npos)
    r = np.linspace(0, 1, 101)
    precision = np.interp(r, rec, prec, right=0)
    confidence = np.interp(r, rec, score, right=0)
    curves = np.ones((5, 101))
    if errs is not None:
        mconf = score[tp]
        for e in range(5):
            cm = _cummean(errs[tp, e])
            curves[e] = np.interp(confidence[::-1], mconf[::-1], cm[::-1])[::-1]
    return precision, confidence, curves


def _calc_ap(precision):
    return float(np.mean(np.maximum(precision[FIRST_IND:] - MIN_PRECISION, 0.0)) / (1.0 - MIN_PRECISION))


def _calc_tp(confidence, curve):
    nz = np.nonzero(confidence)[0]
    last = int(nz[-1]) if len(nz) else 0
    return 1.0 if last < FIRST_IND else float(np.mean(curve[FIRST_IND:last + 1]))


# ----------------------------------------------------------------------------------- the metric
class NuScenesDetectionScore:
    """nuScenes mAP, true-positive errors and NDS over the frames given to `update`.

    class_names: the detector's classes, label k <-> class_names[k] (default: center_head.NUS_TASKS flattened).
    class_range: {name: metres} for classes outside the nuScenes range table, or to override it.
    `compute()` -> {"NuScenes/{class}_AP_dist_{0.5|1.0|2.0|4.0}", "NuScenes/{class}_{trans|scale|orient|vel|attr}_err",
    "NuScenes/mAP", "NuScenes/mATE", "mASE", "mAOE", "mAVE", "mAAE", "NuScenes/NDS"}. Errors that are not defined
    for a class (traffic_cone: attr, vel, orient; barrier: attr, vel) are NaN and left out of the means. The
    accumulator (the frames' tensors) stays on the detections' device."""

    def __init__(self, class_names=None, class_range=None):
        self.class_names = [n for t in NUS_TASKS for n in t] if class_names is None else list(class_names)
        if not self.class_names:
            raise ValueError("NuScenesDetectionScore needs at least one class name")
        cr = dict(class_range or {})
        self.class_range = []
        for n in self.class_names:
            if n in cr:
                self.class_range.append(float(cr[n]))
            elif n in CLASS_RANGE:
                self.class_range.append(CLASS_RANGE[n])
            else:
                raise ValueError(f"class {n!r} is not in the nuScenes range table: pass class_range={{{n!r}: metres}}")
        self.reset()

    def reset(self):
        self._det, self._gt = [], []     # one tuple of concatenated tensors per update() call
        self._nd, self._ng = [], []      # detections / ground truths of every frame
        self._device = None

    def __len__(self):
        return len(self._nd)

    # ------------------------------------------------------------------ per-class tables as tensors
    def _table(self, values, dtype, dev):
        return torch.tensor(list(values), dtype=dtype, device=dev)

    def _default_attr(self, label, box, dev):
        """mmdet3d's attribute rule for detections without attr_labels: by class and speed (float64 of the fp32
        velocities, > 0.2 is moving)."""
        names = self.class_names
        default = self._table([_attr_id(DEFAULT_ATTRIBUTE.get(n)) for n in names] + [-1], torch.int64, dev)
        moving = self._table([_attr_id(_MOVING.get(n, DEFAULT_ATTRIBUTE.get(n))) for n in names] + [-1], torch.int64, dev)
        still = self._table([_attr_id(_STILL.get(n, DEFAULT_ATTRIBUTE.get(n))) for n in names] + [-1], torch.int64, dev)
        C = len(names)
        k = torch.where((label >= 0) & (label < C), label, torch.full_like(label, C))
        v = box[:, 7:9].double()
        speed = torch.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
        return torch.where(speed > MOVING_SPEED, moving[k], still[k])

    def update(self, preds, gts):
        """preds: the per-frame dicts of `predict` (bboxes_3d [n, 7+], scores_3d, labels_3d; optional attr_labels,
        indices into ATTRIBUTES or -1). gts: per frame a dict with bboxes_3d [m, 7+] and labels_3d (int64; -1: no
        class) and optionally num_pts (0: dropped), attr_labels (-1: none), ego_origin (x, y of the ego origin in
        LiDAR coordinates); or a (boxes, labels) pair. Missing fields: num_pts positive, attributes -1, origin
        (0, 0). More than 500 detections or NUS_MAX_GT ground truths in a frame raise ValueError, and nothing of
        that call is kept."""
        if len(preds) != len(gts):
            raise ValueError(f"{len(preds)} frames of detections, {len(gts)} of ground truth")
        dets, truths = [], []
        device = self._device
        for p, g in zip(preds, gts):
            box = p["bboxes_3d"]
            box = getattr(box, "tensor", box)
            if device is None:
                device = box.device     # the accumulator lives where the first detections do
            n = box.shape[0]
            if n > MAX_BOXES_PER_SAMPLE:
                raise ValueError(f"a frame has {n} detections; nuScenes takes at most {MAX_BOXES_PER_SAMPLE}")
            f32 = dict(dtype=torch.float32, device=device)
            i64 = dict(dtype=torch.int64, device=device)
            label = p["labels_3d"].detach().reshape(n).to(**i64)
            box9 = _box9(box.detach().reshape(n, box.shape[-1]), f32)
            attr = p.get("attr_labels")
            attr = self._default_attr(label, box9, device) if attr is None else torch.as_tensor(attr).reshape(n).to(**i64)
            if isinstance(g, (tuple, list)):
                g = dict(bboxes_3d=g[0], labels_3d=g[1])
            gb = _field(g, ("bboxes_3d", "gt_bboxes_3d", "boxes"))
            gb = torch.as_tensor(getattr(gb, "tensor", gb))
            m = gb.shape[0]
            if m > _ffi.NUS_MAX_GT:
                raise ValueError(f"a frame has {m} ground truths; the evaluator takes at most {_ffi.NUS_MAX_GT}")

            def opt(names, fill):
                v = _field(g, names)
                return torch.full((m,), fill, **i64) if v is None else torch.as_tensor(v).reshape(m).to(**i64)

            ego = _field(g, ("ego_origin",))
            ego = torch.zeros(2, dtype=torch.float64) if ego is None else torch.as_tensor(ego).reshape(-1)[:2].double()
            ego = ego.to(device)
            dets.append((box9, p["scores_3d"].detach().reshape(n).to(**f32), label, attr, ego.expand(n, 2)))
            truths.append((_box9(gb.detach().reshape(m, gb.shape[-1]), f32),
                           torch.as_tensor(_field(g, ("labels_3d", "gt_labels_3d", "labels"))).reshape(m).to(**i64),
                           opt(("num_pts", "num_lidar_pts"), 1), opt(("attr_labels", "gt_attr_labels"), -1),
                           ego.expand(m, 2)))
        if dets:   # nothing is kept of a call that raised
            self._device = device
            self._nd += [d[0].shape[0] for d in dets]
            self._ng += [t[0].shape[0] for t in truths]
            self._det.append(tuple(torch.cat([d[k] for d in dets]) for k in range(5)))
            self._gt.append(tuple(torch.cat([t[k] for t in truths]) for k in range(5)))

    # ------------------------------------------------------------------ pieces (the tests call them)
    def _keep(self, box, label, ego, dev):
        """Inside the class range: hypot(x - ex, y - ey) < class_range[label], decided on the squares in float64
        (exact for fp32 coordinates, so it decides as the real-number comparison does)."""
        C = len(self.class_names)
        r = self._table(self.class_range + [0.0], torch.float64, dev)
        k = torch.where((label >= 0) & (label < C), label, torch.full_like(label, C))
        dx, dy = box[:, 0].double() - ego[:, 0], box[:, 1].double() - ego[:, 1]
        return (label >= 0) & (label < C) & (dx * dx + dy * dy < r[k] * r[k])

    def _matches(self, detail=None, thresholds=DIST_THS):
        """-> match [n_thr, n_det] int32 (the global ground-truth row each detection took at each threshold, or
        -1), err [n_det, 5] (the errors of the matches at DIST_TH_TP; NaN rows elsewhere) and order [n_det] int64
        (the detections' global indices in evaluation order: descending score, equal scores by descending
        index), all on the CPU and indexed by the detections' global index (the order of `update`, then the row).
        detail: a dict that receives the flat inputs (scores, labels, keep flags, offsets)."""
        thr = [float(t) for t in thresholds]
        if DIST_TH_TP not in thr:
            raise ValueError(f"the thresholds must hold the true-positive threshold {DIST_TH_TP}")
        dev = self._device if self._device is not None else torch.device("cpu")
        C = len(self.class_names)
        det_off, gt_off = _offsets(self._nd), _offsets(self._ng)
        n_det, n_gt, F = det_off[-1], gt_off[-1], len(self._nd)
        f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
        box0, ego0 = torch.zeros((0, 9), **f32), torch.zeros((0, 2), dtype=torch.float64, device=dev)
        no_det = ((box0, torch.zeros(0, **f32), torch.zeros(0, **i64), torch.zeros(0, **i64), ego0),)
        no_gt = ((box0, torch.zeros(0, **i64), torch.zeros(0, **i64), torch.zeros(0, **i64), ego0),)
        det, score, dl, da, de = (torch.cat([d[k] for d in (self._det or no_det)]).contiguous() for k in range(5))
        gt, gl, gn, ga, ge = (torch.cat([g[k] for g in (self._gt or no_gt)]).contiguous() for k in range(5))
        dkeep = self._keep(det, dl, de, dev)
        gkeep = self._keep(gt, gl, ge, dev) & (gn != 0)
        # evaluation order: descending score, equal scores by descending global index (a stable descending sort
        # of the reversed list), then grouped by frame with that order kept inside each frame
        order = (n_det - 1) - torch.sort(score.flip(0), descending=True, stable=True)[1]
        frame = torch.repeat_interleave(torch.arange(F, device=dev), torch.tensor(self._nd, **i64), output_size=n_det) \
            if F else torch.zeros(0, **i64)
        perm = order[torch.sort(frame[order], stable=True)[1]]
        period = torch.where(dl == (self.class_names.index("barrier") if "barrier" in self.class_names else -2),
                             torch.tensor(math.pi, **f32), torch.tensor(2 * math.pi, **f32))
        i32 = dict(dtype=torch.int32, device=dev)
        dev_off = (torch.tensor(det_off, **i32), torch.tensor(gt_off, **i32)) if det.is_cuda else None
        match_p = center_matches(det[perm, :2], dl[perm], dkeep[perm], det_off, gt[:, :2], gl, gkeep, gt_off, C, thr,
                                 _dev_off=dev_off)
        match = torch.empty_like(match_p)
        match[:, perm] = match_p
        err = _tp_errors(det, gt, match[thr.index(DIST_TH_TP)].contiguous(), period, da.to(torch.int32).contiguous(),
                         ga.to(torch.int32).contiguous())
        npos = torch.bincount(gl[gkeep], minlength=C)[:C] if n_gt else torch.zeros(C, **i64)
        if det.is_cuda:
            # the one host read: everything the curves need, as one int32 buffer
            T = len(thr)
            buf = torch.cat([match.reshape(-1), err.reshape(-1).view(torch.int32), score.view(torch.int32),
                             dl.to(torch.int32), dkeep.to(torch.int32), order.to(torch.int32),
                             npos.to(torch.int32)]).cpu()
            parts = torch.split(buf, [T * n_det, 5 * n_det, n_det, n_det, n_det, n_det, C])
            match, err = parts[0].view(T, n_det), parts[1].view(torch.float32).view(n_det, 5)
            score, dl, dkeep, order, npos = (parts[2].view(torch.float32), parts[3].long(), parts[4] != 0,
                                             parts[5].long(), parts[6].long())
        if detail is not None:
            detail.update(score=score, label=dl, keep=dkeep, npos=npos, det_off=det_off, gt_off=gt_off,
                          thresholds=thr)
        return match, err, order

    def compute(self) -> dict:
        names, C = self.class_names, len(self.class_names)
        detail = {}
        match, err, order = self._matches(detail)
        thr = detail["thresholds"]
        score = detail["score"].double().numpy()[order.numpy()]
        label = detail["label"].numpy()[order.numpy()]
        keep = detail["keep"].numpy()[order.numpy()]
        match = match.numpy()[:, order.numpy()]
        err = err.double().numpy()[order.numpy()]
        npos = detail["npos"].tolist()
        out, aps = {}, []
        tps = np.full((C, 5), np.nan)
        for c, name in enumerate(names):
            sel = keep & (label == c)
            sc, er = score[sel], err[sel]
            for t, th in enumerate(thr):
                tp = match[t][sel] >= 0
                want_err = th == DIST_TH_TP
                precision, confidence, curves = _curves(tp, sc, npos[c], er if want_err else None)
                ap = _calc_ap(precision)
                aps.append(ap)
                out[f"NuScenes/{name}_AP_dist_{th}"] = ap
                if want_err:
                    for e, m in enumerate(TP_METRICS):
                        if m not in UNDEFINED.get(name, ()):
                            tps[c, e] = _calc_tp(confidence, curves[e])
            for e, m in enumerate(TP_METRICS):
                out[f"NuScenes/{name}_{m}_err"] = float(tps[c, e])
        out["NuScenes/mAP"] = float(np.mean(aps))
        total = 5.0 * out["NuScenes/mAP"]
        for e, m in enumerate(MEAN_NAMES):
            col = tps[:, e][~np.isnan(tps[:, e])]
            mean = float(col.mean()) if len(col) else math.nan
            out[f"NuScenes/{m}"] = mean
            total += 1.0 - min(1.0, mean)     # a mean over nothing (NaN) scores 0, as min(1, NaN) does
        out["NuScenes/NDS"] = total / 10.0
        return out


def _box9(box, kw):
    """[n, 7+] -> [n, 9] fp32: missing velocity columns count as 0."""
    box = box.to(**kw)
    if box.shape[-1] < 7:
        raise ValueError(f"boxes need at least 7 columns, got {box.shape[-1]}")
    if box.shape[-1] >= 9:
        return box[:, :9].contiguous()
    return torch.cat([box[:, :7], box.new_zeros((box.shape[0], 9 - 7))], dim=1)
