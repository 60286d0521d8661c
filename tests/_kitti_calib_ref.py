"""Float64 restatement of the calibration side of the KITTI evaluator (DESIGN.md "KITTI average precision",
"Calibration": projection, validity, clipping, observation angle, 2D IoU, the DontCare ratio, the matcher with
stuff detections and the orientation similarity) as plain loops. It restates the specification, not the product
code, and imports nothing from the package; the BEV / 3D side is tests/_kitti_eval_ref.py's.

`project_f32` and `iou_2d_f32` / `dc_ratio_f32` run the same operations in the same order in numpy float32: the
independent fp32 yardstick the GPU tests take their tolerances from.
"""
from __future__ import annotations

import math

import numpy as np

from tests import _kitti_eval_ref as kref

PCD_LIMIT_RANGE = (0, -40, -3, 70.4, 40, 0.0)
ALL_METRICS = ("BEV", "3D", "2D", "AOS")
SIM_ONE = float(1 << 40)


# ----------------------------------------------------------------------------------- calibration
def lidar2img(P2, R0_rect, Tr_velo_to_cam):
    P = [[float(v) for v in row] for row in np.asarray(P2).reshape(3, 4)]
    R = [[float(np.asarray(R0_rect).reshape(3, 3)[i][j]) if i < 3 and j < 3 else float(i == j) for j in range(4)]
         for i in range(4)]
    T = [[float(v) for v in row] for row in np.asarray(Tr_velo_to_cam).reshape(3, 4)] + [[0.0, 0.0, 0.0, 1.0]]
    RT = [[sum(R[i][k] * T[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    return np.array([[sum(P[i][k] * RT[k][j] for k in range(4)) for j in range(4)] for i in range(3)],
                    dtype=np.float64).astype(np.float32)


def corners(box):
    """The 8 corners of (x, y, z, dx, dy, dz, yaw), z the bottom face, in float64."""
    x, y, z, dx, dy, dz, yaw = (float(v) for v in box[:7])
    s, c = math.sin(yaw), math.cos(yaw)
    out = []
    for k in range(8):
        lx = -dx / 2 if k & 1 else dx / 2
        ly = -dy / 2 if k & 2 else dy / 2
        out.append((x + lx * c - ly * s, y + lx * s + ly * c, z + dz if k & 4 else z))
    return out


def project(box, mat, hw, rng=PCD_LIMIT_RANGE):
    """One box -> dict(raw [4], clip [4], valid, alpha, height, w = the 8 corners' W) in float64. A box with a
    corner whose u or v is not finite has four NaNs as its raw box and (0, 0, 0, 0) as its clipped box."""
    m = [float(v) for v in np.asarray(mat, dtype=np.float64).reshape(-1)[:12]]
    h, w = float(hw[0]), float(hw[1])
    us, vs, ws = [], [], []
    for cx, cy, cz in corners(box):
        X, Y, W = (m[4 * a] * cx + m[4 * a + 1] * cy + m[4 * a + 2] * cz + m[4 * a + 3] for a in range(3))
        with np.errstate(all="ignore"):
            us.append(float(np.float64(X) / np.float64(W)))
            vs.append(float(np.float64(Y) / np.float64(W)))
        ws.append(W)
    x, y, z, yaw = float(box[0]), float(box[1]), float(box[2]), float(box[6])
    alpha = math.atan2(y, x) - yaw - math.pi / 2 if x == x and y == y else math.nan
    if not all(math.isfinite(v) for v in us + vs):
        return dict(raw=[math.nan] * 4, clip=[0.0] * 4, valid=False, alpha=alpha, height=0.0, w=ws)
    raw = [min(us), min(vs), max(us), max(vs)]
    clip = [min(max(raw[0], 0.0), w), min(max(raw[1], 0.0), h), min(max(raw[2], 0.0), w), min(max(raw[3], 0.0), h)]
    valid = (raw[0] < w and raw[1] < h and raw[2] > 0 and raw[3] > 0 and rng[0] < x < rng[3] and rng[1] < y < rng[4]
             and rng[2] < z < rng[5])
    return dict(raw=raw, clip=clip, valid=bool(valid), alpha=alpha, height=clip[3] - clip[1], w=ws)


def project_f32(boxes, mats, hws):
    """n boxes [n, 7], each with its own matrix mats [n, 12] and image hws [n, 2], in numpy float32, every operation
    rounded in the specification's order. -> dict(raw, clip [n, 4], alpha, height [n]) float32."""
    f = np.float32
    b = np.asarray(boxes, dtype=f).reshape(-1, 7)
    M = np.asarray(mats, dtype=f).reshape(-1, 12)
    H, W = np.asarray(hws, dtype=f).reshape(-1, 2).T
    x, y, z, dx, dy, dz, yaw = b.T
    with np.errstate(all="ignore"):
        s, c = np.sin(yaw), np.cos(yaw)
        hx, hy, zt = dx * f(0.5), dy * f(0.5), z + dz
        us, vs = [], []
        for k in range(8):
            lx, ly, cz = (-hx if k & 1 else hx), (-hy if k & 2 else hy), (zt if k & 4 else z)
            cx = x + lx * c - ly * s
            cy = y + lx * s + ly * c
            r = [M[:, 4 * a] * cx + M[:, 4 * a + 1] * cy + M[:, 4 * a + 2] * cz + M[:, 4 * a + 3] for a in range(3)]
            us.append(r[0] / r[2])
            vs.append(r[1] / r[2])
        U, V = np.stack(us, 1), np.stack(vs, 1)
        fin = np.isfinite(U).all(1) & np.isfinite(V).all(1)
        raw = np.stack([U.min(1), V.min(1), U.max(1), V.max(1)], 1)
        raw[~fin] = np.nan
        lim = np.stack([W, H, W, H], 1)
        clip = np.where(fin[:, None], np.minimum(np.maximum(raw, f(0)), lim), f(0)).astype(f)
        alpha = np.arctan2(y, x) - yaw - f(math.pi / 2)
    assert raw.dtype == f and clip.dtype == f and alpha.dtype == f
    return dict(raw=raw, clip=clip, alpha=alpha, height=clip[:, 3] - clip[:, 1])


# ----------------------------------------------------------------------------------- 2D overlaps
def _inter(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    return iw * ih if iw > 0 and ih > 0 else 0.0


def iou_2d(a, b):
    """IoU of two (x1, y1, x2, y2) boxes without a +1; exactly 0 when either has a non-positive side."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    if not (a[2] - a[0] > 0 and a[3] - a[1] > 0 and b[2] - b[0] > 0 and b[3] - b[1] > 0):
        return 0.0
    inter = _inter(a, b)
    if not inter > 0:
        return 0.0
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def dc_ratio(det, dc):
    """inter(det, dc) / area(det); 0 for a detection of non-positive side."""
    det, dc = [float(v) for v in det], [float(v) for v in dc]
    if not (det[2] - det[0] > 0 and det[3] - det[1] > 0):
        return 0.0
    return _inter(dc, det) / ((det[2] - det[0]) * (det[3] - det[1]))


def iou_matrix(dets, gts):
    dets, gts = np.asarray(dets, dtype=np.float64).reshape(-1, 4), np.asarray(gts, dtype=np.float64).reshape(-1, 4)
    return np.array([[iou_2d(g, d) for g in gts] for d in dets], dtype=np.float64).reshape(len(dets), len(gts))


def dc_matrix(dets, dcs):
    dets, dcs = np.asarray(dets, dtype=np.float64).reshape(-1, 4), np.asarray(dcs, dtype=np.float64).reshape(-1, 4)
    return np.array([[dc_ratio(d, c) for c in dcs] for d in dets], dtype=np.float64).reshape(len(dets), len(dcs))


def _pairs_f32(dets, others):
    f = np.float32
    d = np.asarray(dets, dtype=f).reshape(-1, 1, 4)
    g = np.asarray(others, dtype=f).reshape(1, -1, 4)
    iw = np.minimum(d[..., 2], g[..., 2]) - np.maximum(d[..., 0], g[..., 0])
    ih = np.minimum(d[..., 3], g[..., 3]) - np.maximum(d[..., 1], g[..., 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, f(0))
    wd, hd, wg, hg = d[..., 2] - d[..., 0], d[..., 3] - d[..., 1], g[..., 2] - g[..., 0], g[..., 3] - g[..., 1]
    return inter, wd, hd, wg, hg


def iou_matrix_f32(dets, gts):
    inter, wd, hd, wg, hg = _pairs_f32(dets, gts)
    ok = (wd > 0) & (hd > 0) & (wg > 0) & (hg > 0) & (inter > 0)
    with np.errstate(all="ignore"):
        v = inter / ((wg * hg + wd * hd) - inter)
    out = np.where(ok, v, np.float32(0))
    assert out.dtype == np.float32
    return out


def dc_matrix_f32(dets, dcs):
    inter, wd, hd, _, _ = _pairs_f32(dets, dcs)
    with np.errstate(all="ignore"):
        v = inter / (wd * hd)
    out = np.where((wd > 0) & (hd > 0), v, np.float32(0)) + np.zeros_like(inter)
    assert out.dtype == np.float32
    return out


# ----------------------------------------------------------------------------------- matching
def similarity(alpha_gt, alpha_det):
    return (1.0 + math.cos(float(alpha_gt) - float(alpha_det))) / 2.0


def match_frame(ov, score, flag_det, flag_gt, min_ov, thresh, stuff=None, alpha_det=None, alpha_gt=None):
    """The count pass of compute_statistics_jit for metric 0 (2D bbox) on one frame: ov[j][i] detection j, ground
    truth i. A stuff detection takes part in the matching but is no false positive; every true positive adds its
    orientation similarity. -> tp, fp, fn, similarity sum, [the (gt, det) pairs of the true positives]."""
    nd = len(score)
    assigned = [False] * nd
    ignored_thr = [bool(score[j] < thresh) for j in range(nd)]
    tp = fp = fn = 0
    sim = 0.0
    pairs = []
    for i in range(len(flag_gt)):
        if flag_gt[i] == -1:
            continue
        det, valid, max_ov, took_ignored = -1, False, 0, False
        for j in range(nd):
            if flag_det[j] == -1 or assigned[j] or ignored_thr[j]:
                continue
            o = ov[j][i]
            if o > min_ov and (o > max_ov or took_ignored) and flag_det[j] == 0:
                max_ov, det, valid, took_ignored = o, j, True, False
            elif o > min_ov and not valid and flag_det[j] == 1:
                det, valid, took_ignored = j, True, True
        if not valid and flag_gt[i] == 0:
            fn += 1
        elif valid and (flag_gt[i] == 1 or flag_det[det] == 1):
            assigned[det] = True
        elif valid:
            tp += 1
            assigned[det] = True
            pairs.append((i, det))
            if alpha_det is not None:
                sim += similarity(alpha_gt[i], alpha_det[det])
    for j in range(nd):
        if assigned[j] or flag_det[j] in (-1, 1) or ignored_thr[j]:
            continue
        if stuff is not None and stuff[j]:
            continue
        fp += 1
    return tp, fp, fn, sim, pairs


def average_orientation(counts, sims):
    """counts [(tp, fp, fn)], sims [similarity sum] per threshold -> (AOS11, AOS40)."""
    a = [0.0] * 41
    for k, ((tp, fp, _), s) in enumerate(zip(counts, sims)):
        a[k] = s / (tp + fp) if tp + fp else 0.0
    for k in range(41):
        a[k] = max(a[k:])
    return 100.0 * sum(a[0::4]) / 11.0, 100.0 * sum(a[1:]) / 40.0


# ----------------------------------------------------------------------------------- the whole metric
def prepare(frames, rng=PCD_LIMIT_RANGE):
    """Apply the calibration to kref-style frames that carry lidar2img [3, 4] / img_shape (and optionally gt_bbox
    [ng, 4], gt_alpha, gt_height_given = False, dontcare [k, 4]): invalid detections are REMOVED, heights, 2D
    boxes and angles filled in. -> new frames with det_box2d, gt_box2d, det_alpha, gt_alpha, det_keep (indices)."""
    out = []
    for fr in frames:
        g = dict(fr)
        mat, hw = fr["lidar2img"], fr["img_shape"]
        pd = [project(b, mat, hw, rng) for b in fr["det_boxes"]]
        pg = [project(b, mat, hw, rng) for b in fr["gt_boxes"]]
        keep = [j for j, p in enumerate(pd) if p["valid"]]
        for k in ("det_boxes", "det_scores", "det_labels"):
            g[k] = fr[k][keep]
        g["det_keep"] = keep
        g["det_height"] = np.array([pd[j]["height"] for j in keep], dtype=np.float64)
        g["det_box2d"] = np.array([pd[j]["clip"] for j in keep], dtype=np.float64).reshape(len(keep), 4)
        g["det_alpha"] = np.array([pd[j]["alpha"] for j in keep], dtype=np.float64)
        gb = fr.get("gt_bbox")
        g["gt_box2d"] = (np.asarray(gb, dtype=np.float64) if gb is not None
                         else np.array([p["clip"] for p in pg], dtype=np.float64)).reshape(len(pg), 4)
        if not fr.get("gt_height_given", True):
            g["gt_height"] = g["gt_box2d"][:, 3] - g["gt_box2d"][:, 1]
        ga = fr.get("gt_alpha")
        g["gt_alpha"] = (np.asarray(ga, dtype=np.float64) if ga is not None
                         else np.array([p["alpha"] for p in pg], dtype=np.float64))
        out.append(g)
    return out


def evaluate(frames, class_names, metrics=ALL_METRICS, min_overlaps=None, overlaps=None, ov2d=None, alphas=None,
             stuffs=None):
    """frames: `prepare`d frames. -> {(metric name, c, d, t): dict(counts, ap11, ap40, and for 2D / AOS sims,
    thresholds)}. overlaps: {mode: [per frame]} for BEV / 3D, ov2d: [per frame [nd, ng]], alphas: [per frame
    (det, gt)], stuffs: [per frame [C][nd]] to use instead of the float64 ones."""
    table = dict(kref.KITTI_MIN_OVERLAPS)
    table.update(min_overlaps or {})
    out = {}
    if "BEV" in metrics or "3D" in metrics:
        res = kref.evaluate(frames, class_names, min_overlaps, overlaps)
        for (mode, c, d, t), r in res.items():
            if kref.METRICS[mode] in metrics:
                out[(kref.METRICS[mode], c, d, t)] = r
    if "2D" not in metrics and "AOS" not in metrics:
        return out
    F = len(frames)
    ovs = [np.asarray(o).tolist() for o in ov2d] if ov2d is not None else \
        [iou_matrix(fr["det_box2d"], fr["gt_box2d"]).tolist() for fr in frames]
    als = alphas if alphas is not None else [(fr["det_alpha"], fr["gt_alpha"]) for fr in frames]
    scores = [[float(s) for s in fr["det_scores"]] for fr in frames]
    for c, name in enumerate(class_names):
        mo = float(np.float32(table[name][0]))      # the strict value in both tables
        if stuffs is not None:
            st = [s[c] for s in stuffs]
        else:
            st = []
            for fr in frames:
                dc = np.asarray(fr.get("dontcare", np.zeros((0, 4)))).reshape(-1, 4)
                st.append([any(dc_ratio(b, k) > mo for k in dc) for b in fr["det_box2d"]])
        for d in range(3):
            fds = [[kref.det_flag(int(l), float(h), c, d) for l, h in zip(fr["det_labels"], fr["det_height"])]
                   for fr in frames]
            fgs = [[kref.gt_flag(int(l), int(nb), float(h), float(o), float(t), c, d) for l, nb, h, o, t in
                    zip(fr["gt_labels"], fr["gt_neighbor"], fr["gt_height"], fr["gt_occluded"], fr["gt_truncated"])]
                   for fr in frames]
            n_valid = sum(f.count(0) for f in fgs)
            tps = [kref.match_frame(ovs[f], scores[f], fds[f], fgs[f], mo, 0.0, False)[3] for f in range(F)]
            thr = kref.thresholds([s for fr in tps for _, s in fr], n_valid)
            counts, sims = [], []
            for th in thr:
                tot, sim = [0, 0, 0], 0.0
                for f in range(F):
                    r = match_frame(ovs[f], scores[f], fds[f], fgs[f], mo, th, st[f], als[f][0], als[f][1])
                    tot = [tot[0] + r[0], tot[1] + r[1], tot[2] + r[2]]
                    sim += r[3]
                counts.append(tuple(tot))
                sims.append(sim)
            ap11, ap40 = kref.average_precision(counts)
            ao11, ao40 = average_orientation(counts, sims)
            for t in range(2):
                out[("2D", c, d, t)] = dict(tp_scores=tps, thresholds=thr, counts=counts, n_valid_gt=n_valid,
                                            ap11=ap11, ap40=ap40, sims=sims)
                out[("AOS", c, d, t)] = dict(counts=counts, sims=sims, ap11=ao11, ap40=ao40)
    return {k: v for k, v in out.items() if k[0] in metrics}


def result_dict(res, class_names, metrics=ALL_METRICS):
    """The product's result keys from `evaluate`'s output."""
    out = {}
    for (m, c, d, t), r in res.items():
        for name in ("ap11", "ap40"):
            out[f"KITTI/{class_names[c]}_{m}_{name.upper()}_{kref.DIFFICULTIES[d]}_{kref.TABLES[t]}"] = r[name]
    for m in metrics:
        for name in ("AP11", "AP40"):
            for d in range(3):
                vals = [out[f"KITTI/{n}_{m}_{name}_{kref.DIFFICULTIES[d]}_strict"] for n in class_names]
                out[f"KITTI/Overall_{m}_{name}_{kref.DIFFICULTIES[d]}"] = sum(vals) / len(vals)
    return out
