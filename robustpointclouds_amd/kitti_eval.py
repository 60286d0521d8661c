"""KITTI average precision (BEV and 3D, R11 and R40) from the per-frame dicts `predict` returns.

Restates mmdet3d v1.x `evaluation/functional/kitti_utils/eval.py` (`clean_data`, `compute_statistics_jit`,
`get_thresholds`, `eval_class`, `get_mAP11/40`) in the LiDAR frame; the specification is written out in
DESIGN.md "KITTI average precision". Boxes are LiDAR boxes (x, y, z of the BOTTOM face, dx, dy, dz, yaw) as
`predict` returns them; of a 9-column CenterPoint box the first 7 columns are used. The 2D `bbox` / AOS
metrics and DontCare regions are not part of it.

CUDA tensors run on the HIP kernels of csrc/kitti_eval.hip — `rpc_kitti_overlaps` (all frames' overlap
matrices in one launch), `rpc_kitti_match_scores` (matcher pass 1) and `rpc_kitti_match_counts` (pass 2, one
lane per threshold) — with one host read between the passes (how many scores each group emitted: the positions
of the thresholds in the sorted scores depend on nothing else) and one at the end (the counts). CPU tensors
take a plain Python / torch path with the same semantics (slow; like postprocess.py's, it makes the metric
usable and testable without a GPU). Sorting, flags, precision and AP are torch on either path.
"""
from __future__ import annotations

import math

import torch

from . import _ffi
from .postprocess import _iou_cpu

__all__ = ["box_overlaps", "threshold_indices", "KittiAP", "DIFFICULTIES", "MIN_HEIGHT", "MAX_OCCLUSION",
           "MAX_TRUNCATION", "MIN_OVERLAP_STRICT", "MIN_OVERLAP_LOOSE"]

DIFFICULTIES = ("easy", "moderate", "hard")
MIN_HEIGHT = (40.0, 25.0, 25.0)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
MIN_OVERLAP_STRICT = {"Car": 0.7, "Pedestrian": 0.5, "Cyclist": 0.5}
MIN_OVERLAP_LOOSE = {"Car": 0.5, "Pedestrian": 0.25, "Cyclist": 0.25}
TABLES = ("strict", "loose")
METRICS = ("BEV", "3D")
NO = _ffi.KITTI_NO_SCORE
N_THR = _ffi.KITTI_MAX_THR


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


def _match_frame(ov, score, fdet, fgt, min_ov, thresh, count_pass):
    """compute_statistics_jit for one frame: ov[j][i] (lists), score / fdet per detection, fgt per ground
    truth. -> tp, fp, fn, {gt index: score of its true positive}."""
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
    if count_pass:
        fp = sum(1 for j in range(nd) if not (assigned[j] or fdet[j] in (-1, 1) or ignored_thr[j]))
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
    accumulator (the frames' tensors) stays on the detections' device."""

    def __init__(self, class_names, min_overlaps=None):
        self.class_names = list(class_names)
        if not self.class_names:
            raise ValueError("KittiAP needs at least one class name")
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
        self._device = None

    def __len__(self):
        return len(self._nd)

    def update(self, preds, gts):
        """preds: the per-frame dicts of `predict` (bboxes_3d [n, 7+], scores_3d, labels_3d; optional
        bbox_height, the 2D box height in pixels). gts: per frame a dict with bboxes_3d [m, 7+] and labels_3d
        (int64; -1: any other class) and optionally neighbor (int64: the class this object is the neighbour
        class of — Van for Car, Person_sitting for Pedestrian — or -1), bbox_height, occluded, truncated; or a
        (boxes, labels) pair. Missing fields: height +inf, occluded 0, truncated 0, no neighbour."""
        if len(preds) != len(gts):
            raise ValueError(f"{len(preds)} frames of detections, {len(gts)} of ground truth")
        dets, truths = [], []
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
        if dets:   # nothing is kept of a call that raised
            self._nd += [d[0].shape[0] for d in dets]
            self._ng += [t[0].shape[0] for t in truths]
            self._det.append(tuple(torch.cat([d[k] for d in dets]) for k in range(4)))
            self._gt.append(tuple(torch.cat([t[k] for t in truths]) for k in range(6)))

    # ------------------------------------------------------------------ pieces (the tests call them)
    def _flags(self, dl, dh, gl, gn, gh, go, gt_):
        """flag_det [C * 3, n_det], flag_gt [C * 3, n_gt] int8; row c * 3 + d."""
        fd, fg = [], []
        one, zero, neg = (torch.tensor(v, dtype=torch.int8, device=dl.device) for v in (1, 0, -1))
        for c in range(len(self.class_names)):
            for d in range(3):
                vc = torch.where(gl == c, one, torch.where(gn == c, zero, neg))
                ign = (go > MAX_OCCLUSION[d]) | (gt_ > MAX_TRUNCATION[d]) | (gh <= MIN_HEIGHT[d])
                fg.append(torch.where((vc == 1) & ~ign, zero, torch.where((vc == 0) | (ign & (vc == 1)), one, neg)))
                fd.append(torch.where(dh < MIN_HEIGHT[d], one, torch.where(dl == c, zero, neg)))
        return torch.stack(fd).contiguous(), torch.stack(fg).contiguous()

    def _min_ov(self, dev):
        """[C * 3 * 2] fp32; group (c * 3 + d) * 2 + table."""
        return torch.tensor([self.min_overlaps[c][t] for c in range(len(self.class_names)) for _ in range(3)
                             for t in range(2)], dtype=torch.float32, device=dev)

    def compute(self) -> dict:
        C = len(self.class_names)
        G = C * 3 * 2
        keys = [(m, c, d, t) for m in range(2) for c in range(C) for d in range(3) for t in range(2)]
        ap11 = ap40 = [0.0] * (2 * G)
        if self._nd:
            counts, nthr = self._counts()
            ap11, ap40 = _average_precision(counts, nthr)
        out = {}
        for (m, c, d, t), a11, a40 in zip(keys, ap11, ap40):
            for name, v in (("AP11", a11), ("AP40", a40)):
                out[f"KITTI/{self.class_names[c]}_{METRICS[m]}_{name}_{DIFFICULTIES[d]}_{TABLES[t]}"] = float(v)
        for m in range(2):
            for name in ("AP11", "AP40"):
                for d in range(3):
                    vals = [out[f"KITTI/{n}_{METRICS[m]}_{name}_{DIFFICULTIES[d]}_strict"] for n in self.class_names]
                    out[f"KITTI/Overall_{METRICS[m]}_{name}_{DIFFICULTIES[d]}"] = float(sum(vals) / len(vals))
        return out

    def _counts(self, overlaps=None, detail=None):
        """-> counts [2 * G, 41, 3] int64 (tp, fp, fn; CPU) and nthr [2 * G] (list); metric-major groups.
        overlaps: (ov_bev, ov_3d) to use instead of the computed ones; detail: a dict that receives the
        intermediate results (overlaps, pass-1 scores, thresholds)."""
        dev = self._device
        det_off, gt_off = _offsets(self._nd), _offsets(self._ng)
        F = len(self._nd)
        maxd, maxg = _check_caps(det_off, gt_off)
        ov_off = _offsets([(det_off[f + 1] - det_off[f]) * (gt_off[f + 1] - gt_off[f]) for f in range(F)])
        det, score, dl, dh = (torch.cat([d[k] for d in self._det]).contiguous() for k in range(4))
        gt, gl, gn, gh, go, gtr = (torch.cat([g[k] for g in self._gt]).contiguous() for k in range(6))
        fdet, fgt = self._flags(dl, dh, gl, gn, gh, go, gtr)
        min_ov = self._min_ov(dev)
        G = min_ov.numel()
        n_det, n_gt = det_off[-1], gt_off[-1]
        cuda = det.is_cuda
        dev_off = _device_offsets(det_off, gt_off, ov_off, dev) if cuda else None
        if overlaps is None:
            overlaps = [_overlaps(det, det_off, gt, gt_off, ov_off, maxd, maxg, m, dev_off) for m in range(2)]
        frame = (det_off, gt_off, ov_off, maxd, maxg, dev_off)
        # pass 1: the true-positive scores of every group, both metrics
        tps = torch.stack([_match_scores(ov, frame, score, fdet, fgt, min_ov) for ov in overlaps])   # [2, G, n_gt]
        srt = tps.sort(dim=-1, descending=True)[0]
        nemit = (tps > NO).sum(-1).reshape(-1)
        nvalid = (fgt == 0).sum(-1)
        host = torch.cat([nemit, nvalid]).cpu().tolist()            # the one host read between the passes
        nemit, nvalid = host[:2 * G], host[2 * G:]
        idx = [threshold_indices(nemit[q], nvalid[(q % G) // 2]) for q in range(2 * G)]
        nthr = [len(v) for v in idx]
        pad = torch.tensor([v + [0] * (N_THR - len(v)) for v in idx], dtype=torch.int64, device=dev).view(2, G, N_THR)
        if n_gt:
            thr = srt.gather(-1, pad).contiguous()
        else:
            thr = torch.zeros((2, G, N_THR), dtype=torch.float32, device=dev)
        nthr_t = torch.tensor(nthr, dtype=torch.int32, device=dev).view(2, G)
        # pass 2: tp / fp / fn at every threshold
        counts = torch.stack([_match_counts(ov, frame, score, fdet, fgt, min_ov, thr[m], nthr_t[m])
                              for m, ov in enumerate(overlaps)]).reshape(2 * G, N_THR, 3)
        if detail is not None:
            detail.update(overlaps=overlaps, ov_off=ov_off, det_off=det_off, gt_off=gt_off, tp_scores=tps, thr=thr,
                          nthr=nthr, flag_det=fdet, flag_gt=fgt, min_ov=min_ov, score=score, n_valid_gt=nvalid)
        return counts.cpu().to(torch.int64), nthr


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


def _match_counts(ov, frame, score, fdet, fgt, min_ov, thr, nthr):
    """Matcher pass 2 -> counts [G, 41, 3] int32 (tp, fp, fn) summed over the frames."""
    det_off, gt_off, ov_off, maxd, maxg, dev_off = frame
    G = min_ov.numel()
    ntab = G // fdet.shape[0]
    n_det, n_gt = det_off[-1], gt_off[-1]
    if not score.is_cuda:
        out = torch.zeros((G, N_THR, 3), dtype=torch.int32)
        sl, mo, tl, nl = score.tolist(), min_ov.tolist(), thr.tolist(), nthr.tolist()
        for g in range(G):
            if not nl[g]:
                continue
            fr, gr = fdet[g // ntab].tolist(), fgt[g // ntab].tolist()
            for o, s, fd, fg, _ in _frames_cpu(ov, ov_off, det_off, gt_off, sl, fr, gr):
                for k in range(nl[g]):
                    tp, fp, fn, _e = _match_frame(o, s, fd, fg, mo[g], tl[g][k], True)
                    out[g, k, 0] += tp
                    out[g, k, 1] += fp
                    out[g, k, 2] += fn
        return out
    out = torch.empty((G, N_THR, 3), dtype=torch.int32, device=score.device)
    thr, nthr = thr.contiguous(), nthr.contiguous()
    d_off, g_off, o_off = dev_off
    _ffi.check(_ffi.load().rpc_kitti_match_counts(
        _ffi.ptr(ov), _ffi.ptr(o_off), _ffi.ptr(d_off), _ffi.ptr(g_off), len(det_off) - 1, maxd, maxg,
        _ffi.ptr(score), _ffi.ptr(fdet), _ffi.ptr(fgt), n_det, n_gt, _ffi.ptr(min_ov), G, ntab, _ffi.ptr(thr),
        _ffi.ptr(nthr), _ffi.ptr(out), _ffi.stream_of(score)), "rpc_kitti_match_counts")
    return out


def _average_precision(counts, nthr):
    """counts [Q, 41, 3] int64 (CPU), nthr [Q] -> (AP11 [Q], AP40 [Q]) lists of floats. precision[k] =
    tp / (tp + fp) at threshold k (0 beyond the group's thresholds, and where nothing was detected), then the
    running maximum from the right; AP11 = 100 * sum(precision[0::4]) / 11, AP40 = 100 * sum(precision[1:]) / 40."""
    c = counts.double()
    tp, fp = c[..., 0], c[..., 1]
    live = torch.arange(N_THR)[None, :] < torch.tensor(nthr)[:, None]
    prec = torch.where(live & (tp + fp > 0), tp / (tp + fp).clamp(min=1), torch.zeros_like(tp))
    prec = prec.flip(-1).cummax(-1)[0].flip(-1)
    ap11 = (100.0 * prec[:, 0::4].sum(-1) / 11.0).tolist()
    ap40 = (100.0 * prec[:, 1:].sum(-1) / 40.0).tolist()
    return ap11, ap40
