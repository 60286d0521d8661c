"""Float64 restatement of the KITTI BEV / 3D average-precision specification (DESIGN.md "KITTI average
precision", from mmdet3d v1.x kitti_utils/eval.py) as plain loops. It restates the specification, not the
product code, and imports nothing from the package; the rotated-box clipping is tests/_postprocess_ref.py's.

`overlap(a, b, mode, dtype=np.float32)` runs the same algorithm in numpy float32 scalars: the independent fp32
reference the GPU test takes its tolerance from, like `bev_iou(..., np.float32)`.
"""
from __future__ import annotations

import math

import numpy as np

from tests import _postprocess_ref as pref

NO = -10000000
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
DIFFICULTIES = ("easy", "moderate", "hard")
TABLES = ("strict", "loose")
METRICS = ("BEV", "3D")
KITTI_MIN_OVERLAPS = {"Car": (0.7, 0.5), "Pedestrian": (0.5, 0.25), "Cyclist": (0.5, 0.25)}


# ----------------------------------------------------------------------------------- overlaps
def _footprints(a, b, dtype):
    """(intersection area, area a, area b) of the BEV footprints of two (x, y, z, dx, dy, dz, yaw) boxes."""
    if dtype == np.float64:
        T, sin, cos = float, math.sin, math.cos
    else:
        T, sin, cos = dtype, np.sin, np.cos
    pa = pref._corners(T(0), T(0), a[3], a[4], a[6], T, sin, cos)
    poly = pref._corners(b[0] - a[0], b[1] - a[1], b[3], b[4], b[6], T, sin, cos)
    for k in range(4):
        poly = pref._clip_halfplane(poly, pa[k], pa[(k + 1) % 4], T)
        if not poly:
            break
    inter = pref._shoelace(poly, T) if len(poly) >= 3 else T(0)
    area_a, area_b = a[3] * a[4], b[3] * b[4]
    return min(inter, area_a, area_b), area_a, area_b


def overlap(a, b, mode, dtype=np.float64):
    """mode 0: rotated BEV IoU of the footprints; mode 1: 3D IoU (z is the bottom face: the box spans
    [z, z + dz]). 0 if any of the six extents is <= 0."""
    T = float if dtype == np.float64 else dtype
    a = [T(v) for v in np.asarray(a, dtype=dtype)[:7]]
    b = [T(v) for v in np.asarray(b, dtype=dtype)[:7]]
    if not all(v > 0 for v in (a[3], a[4], a[5], b[3], b[4], b[5])):
        return T(0)
    inter, area_a, area_b = _footprints(a, b, dtype)
    if mode == 0:
        v = inter / (area_a + area_b - inter)
    else:
        h = min(a[2] + a[5], b[2] + b[5]) - max(a[2], b[2])
        if not h > 0:
            return T(0)
        va, vb = area_a * a[5], area_b * b[5]
        i3 = min(inter * h, va, vb)
        v = i3 / (va + vb - i3)
    return min(max(v, T(0)), T(1))


_W = 12   # vertex slots of the array form (a quadrilateral clipped by four half-planes has at most 8)


def _corners_v(x, y, dx, dy, yaw, T):
    c, s = np.cos(yaw), np.sin(yaw)
    hx, hy = dx / T(2), dy / T(2)
    px, py = [], []
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        lx, ly = T(sx) * hx, T(sy) * hy
        px.append(x + lx * c - ly * s)
        py.append(y + lx * s + ly * c)
    return np.stack(px, 1), np.stack(py, 1)


def _clip_v(px, py, n, p0, p1, q0, q1, T):
    rows = np.arange(len(n))
    ox, oy, on = np.zeros_like(px), np.zeros_like(py), np.zeros_like(n)
    side = lambda x, y: (q0 - p0) * (y - p1) - (q1 - p1) * (x - p0)
    last = np.maximum(n - 1, 0)
    prx, pry = px[rows, last], py[rows, last]
    for k in range(_W):
        act = k < n
        cx, cy = px[:, k], py[:, k]
        sc, sp = side(cx, cy), side(prx, pry)
        cross = act & ((sc >= T(0)) != (sp >= T(0)))
        with np.errstate(all="ignore"):
            t = sp / (sp - sc)
            ix, iy = prx + t * (cx - prx), pry + t * (cy - pry)
        for sel, vx, vy in ((cross, ix, iy), (act & (sc >= T(0)), cx, cy)):
            r = rows[sel]
            ox[r, on[r]], oy[r, on[r]] = vx[sel], vy[sel]
            on[r] += 1
        prx, pry = np.where(act, cx, prx), np.where(act, cy, pry)
    return ox, oy, on


def overlap_pairs(a, b, mode, dtype=np.float64):
    """`overlap(a[k], b[k], mode, dtype)` for n pairs at once: the same operations in the same order on numpy
    arrays of `dtype` (tests/test_kitti_eval_cpu.py holds the two forms together)."""
    T = dtype
    a = np.asarray(a, dtype=dtype).reshape(-1, 7)
    b = np.asarray(b, dtype=dtype).reshape(-1, 7)
    n = a.shape[0]
    ok = (a[:, 3:6] > 0).all(1) & (b[:, 3:6] > 0).all(1)
    zero = np.zeros(n, dtype=dtype)
    ax, ay = _corners_v(zero, zero, a[:, 3], a[:, 4], a[:, 6], T)
    bx, by = _corners_v(b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 3], b[:, 4], b[:, 6], T)
    px, py = np.zeros((n, _W), dtype=dtype), np.zeros((n, _W), dtype=dtype)
    px[:, :4], py[:, :4] = bx, by
    cnt = np.full(n, 4, dtype=np.int64)
    for k in range(4):
        k1 = (k + 1) % 4
        px, py, cnt = _clip_v(px, py, cnt, ax[:, k], ay[:, k], ax[:, k1], ay[:, k1], T)
    rows = np.arange(n)
    s = np.zeros(n, dtype=dtype)
    last = np.maximum(cnt - 1, 0)
    prx, pry = px[rows, last], py[rows, last]
    for k in range(_W):
        act = k < cnt
        s = np.where(act, s + (prx * py[:, k] - px[:, k] * pry), s)
        prx, pry = np.where(act, px[:, k], prx), np.where(act, py[:, k], pry)
    inter = np.where(cnt >= 3, np.abs(s) / T(2), T(0))
    area_a, area_b = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    inter = np.minimum(np.minimum(inter, area_a), area_b)
    with np.errstate(all="ignore"):
        if mode == 0:
            v = inter / (area_a + area_b - inter)
        else:
            h = np.minimum(a[:, 2] + a[:, 5], b[:, 2] + b[:, 5]) - np.maximum(a[:, 2], b[:, 2])
            ok = ok & (h > 0)
            va, vb = area_a * a[:, 5], area_b * b[:, 5]
            i3 = np.minimum(np.minimum(inter * h, va), vb)
            v = i3 / (va + vb - i3)
    v = np.minimum(np.maximum(v, T(0)), T(1))
    return np.where(ok, v, T(0)).astype(dtype)


def overlap_matrix(dets, gts, mode, dtype=np.float64):
    """[nd, ng] with the ground truth as the first box (the clipper's), as the product does."""
    dets = np.asarray(dets).reshape(-1, 7)
    gts = np.asarray(gts).reshape(-1, 7)
    nd, ng = dets.shape[0], gts.shape[0]
    if nd == 0 or ng == 0:
        return np.zeros((nd, ng), dtype=dtype)
    return overlap_pairs(np.tile(gts, (nd, 1)), np.repeat(dets, ng, axis=0), mode, dtype).reshape(nd, ng)


# ----------------------------------------------------------------------------------- flags
def gt_flag(label, neighbor, height, occluded, truncated, c, d):
    valid_class = 1 if label == c else (0 if neighbor == c else -1)
    ignore = occluded > MAX_OCCLUSION[d] or truncated > MAX_TRUNCATION[d] or height <= MIN_HEIGHT[d]
    if valid_class == 1 and not ignore:
        return 0
    if valid_class == 0 or (ignore and valid_class == 1):
        return 1
    return -1


def det_flag(label, height, c, d):
    if height < MIN_HEIGHT[d]:
        return 1
    if label == c:
        return 0
    return -1


# ----------------------------------------------------------------------------------- matching
def match_frame(ov, score, flag_det, flag_gt, min_ov, thresh, count_pass):
    """ov[j][i]: detection j, ground truth i. -> tp, fp, fn, [(gt index, score of its true positive)]."""
    nd = len(score)
    assigned = [False] * nd
    ignored_thr = [bool(count_pass and score[j] < thresh) for j in range(nd)]
    tp = fp = fn = 0
    emitted = []
    for i in range(len(flag_gt)):
        if flag_gt[i] == -1:
            continue
        det, valid, max_ov, took_ignored = -1, NO, 0, False
        for j in range(nd):
            if flag_det[j] == -1 or assigned[j] or ignored_thr[j]:
                continue
            o = ov[j][i]
            if not count_pass and o > min_ov and score[j] > valid:
                det = j
                valid = score[j]
            elif count_pass and o > min_ov and (o > max_ov or took_ignored) and flag_det[j] == 0:
                max_ov = o
                det = j
                valid = 1
                took_ignored = False
            elif count_pass and o > min_ov and valid == NO and flag_det[j] == 1:
                det = j
                valid = 1
                took_ignored = True
        if valid == NO and flag_gt[i] == 0:
            fn += 1
        elif valid != NO and (flag_gt[i] == 1 or flag_det[det] == 1):
            assigned[det] = True
        elif valid != NO:
            tp += 1
            emitted.append((i, score[det]))
            assigned[det] = True
    if count_pass:
        for j in range(nd):
            if not (assigned[j] or flag_det[j] in (-1, 1) or ignored_thr[j]):
                fp += 1
    return tp, fp, fn, emitted


def thresholds(scores, n_valid_gt):
    """get_thresholds: every score is looked at, in descending order."""
    scores = sorted(scores, reverse=True)
    out = []
    cur = 0.0
    n = n_valid_gt
    if n == 0:
        return out
    for i, s in enumerate(scores):
        l = (i + 1) / n
        r = (i + 2) / n if i < len(scores) - 1 else l
        if (r - cur) < (cur - l) and i < len(scores) - 1:
            continue
        out.append(s)
        cur += 1 / 40.0
    return out


def average_precision(counts):
    """counts: [(tp, fp, fn)] per threshold -> (AP11, AP40)."""
    prec = [0.0] * 41
    for k, (tp, fp, _) in enumerate(counts):
        prec[k] = tp / (tp + fp) if tp + fp else 0.0
    for k in range(41):
        prec[k] = max(prec[k:])
    return 100.0 * sum(prec[0::4]) / 11.0, 100.0 * sum(prec[1:]) / 40.0


# ----------------------------------------------------------------------------------- the whole metric
def evaluate(frames, class_names, min_overlaps=None, overlaps=None):
    """frames: dicts of numpy arrays — det_boxes [nd, 7], det_scores, det_labels, det_height, gt_boxes
    [ng, 7], gt_labels, gt_neighbor, gt_height, gt_occluded, gt_truncated. overlaps: {mode: [per frame
    [nd, ng]]} to use instead of the float64 ones. -> {(mode, c, d, t): dict(tp_scores = per frame
    [(gt index, score)], thresholds, counts = [(tp, fp, fn)] per threshold, n_valid_gt, ap11, ap40)}."""
    table = dict(KITTI_MIN_OVERLAPS)
    table.update(min_overlaps or {})
    out = {}
    for mode in range(2):
        if overlaps is not None:
            ovs = overlaps[mode]
        else:
            ovs = [overlap_matrix(fr["det_boxes"], fr["gt_boxes"], mode) for fr in frames]
        ovs = [np.asarray(o).tolist() for o in ovs]
        for c, name in enumerate(class_names):
            for d in range(3):
                fds, fgs = [], []
                for fr in frames:
                    fds.append([det_flag(int(l), float(h), c, d) for l, h in zip(fr["det_labels"], fr["det_height"])])
                    fgs.append([gt_flag(int(l), int(nb), float(h), float(o), float(t), c, d) for l, nb, h, o, t in
                                zip(fr["gt_labels"], fr["gt_neighbor"], fr["gt_height"], fr["gt_occluded"],
                                    fr["gt_truncated"])])
                n_valid = sum(f.count(0) for f in fgs)
                scores = [[float(s) for s in fr["det_scores"]] for fr in frames]
                for t in range(2):
                    mo = float(np.float32(table[name][t]))     # the product keeps the table in fp32
                    tps = [match_frame(ovs[f], scores[f], fds[f], fgs[f], mo, 0.0, False)[3]
                           for f in range(len(frames))]
                    thr = thresholds([s for fr in tps for _, s in fr], n_valid)
                    counts = []
                    for th in thr:
                        tot = [0, 0, 0]
                        for f in range(len(frames)):
                            r = match_frame(ovs[f], scores[f], fds[f], fgs[f], mo, th, True)
                            tot = [tot[0] + r[0], tot[1] + r[1], tot[2] + r[2]]
                        counts.append(tuple(tot))
                    ap11, ap40 = average_precision(counts)
                    out[(mode, c, d, t)] = dict(tp_scores=tps, thresholds=thr, counts=counts, n_valid_gt=n_valid,
                                                ap11=ap11, ap40=ap40)
    return out


def result_dict(res, class_names):
    """The product's result keys from `evaluate`'s output."""
    out = {}
    for (mode, c, d, t), r in res.items():
        for name in ("ap11", "ap40"):
            out[f"KITTI/{class_names[c]}_{METRICS[mode]}_{name.upper()}_{DIFFICULTIES[d]}_{TABLES[t]}"] = r[name]
    for mode in range(2):
        for name in ("AP11", "AP40"):
            for d in range(3):
                vals = [out[f"KITTI/{n}_{METRICS[mode]}_{name}_{DIFFICULTIES[d]}_strict"] for n in class_names]
                out[f"KITTI/Overall_{METRICS[mode]}_{name}_{DIFFICULTIES[d]}"] = sum(vals) / len(vals)
    return out
