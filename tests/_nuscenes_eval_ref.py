"""An independent restatement of DESIGN.md "nuScenes detection score" in numpy / plain Python, float64, with the
nuscenes-devkit's structure (filter, `accumulate` per class and threshold with a per-detection loop, `calc_ap`,
`calc_tp`, the NDS of detection_cvpr_2019). It shares no code with robustpointclouds_amd/nuscenes_eval.py; its
`interp` is written out (bisection) and not numpy's.

`dtype=np.float32` runs the distance and the true-positive error arithmetic in float32 (every operation rounded),
the yardstick for the device's fp32 errors; decisions on the inputs of tests/_nuscenes_eval_cases.py are the same in
both precisions.

A frame is a dict: det_boxes [n, 9] f32, det_scores [n] f32, det_labels [n] i64, gt_boxes [m, 9] f32, gt_labels [m]
i64 and optionally det_attr, gt_attr (ids into ATTRIBUTES, -1 none), num_pts, ego (x, y)."""
import bisect
import math

import numpy as np

DIST_THS = (0.5, 1.0, 2.0, 4.0)
TP_TH = 2.0
RANGE = dict(car=50, truck=50, bus=50, trailer=50, construction_vehicle=50, pedestrian=40, motorcycle=40,
             bicycle=40, traffic_cone=30, barrier=30)
ATTRIBUTES = ["cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing",
              "pedestrian.sitting_lying_down", "vehicle.moving", "vehicle.parked", "vehicle.stopped"]
ERRORS = ["trans", "scale", "orient", "vel", "attr"]
MEANS = ["mATE", "mASE", "mAOE", "mAVE", "mAAE"]


def default_attribute(name, vx, vy):
    """mmdet3d's NuScenesMetric rule -> attribute name or None."""
    default = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
               "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
               "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": None,
               "traffic_cone": None}
    if math.sqrt(float(vx) ** 2 + float(vy) ** 2) > 0.2:
        if name in ("car", "construction_vehicle", "bus", "truck", "trailer"):
            return "vehicle.moving"
        if name in ("bicycle", "motorcycle"):
            return "cycle.with_rider"
        return default.get(name)
    if name == "pedestrian":
        return "pedestrian.standing"
    if name == "bus":
        return "vehicle.stopped"
    return default.get(name)


class Box:
    def __init__(self, frame, row, glob, name, box, score=None, attr=-1):
        self.frame, self.row, self.glob, self.name, self.box, self.score, self.attr = frame, row, glob, name, box, score, attr


def load(frames, class_names, class_range=None):
    """-> (all detections [Box] in global order, kept detections, kept ground truths per frame, n_gt)."""
    rng = dict(RANGE)
    rng.update(class_range or {})
    all_det, det, gts = [], [], []
    gd = gg = 0
    for f, fr in enumerate(frames):
        ex, ey = [float(v) for v in fr.get("ego", (0.0, 0.0))]
        n, m = len(fr["det_boxes"]), len(fr["gt_boxes"])
        for j in range(n):
            k = int(fr["det_labels"][j])
            name = class_names[k] if 0 <= k < len(class_names) else None
            b = fr["det_boxes"][j]
            if "det_attr" in fr:
                attr = int(fr["det_attr"][j])
            else:
                a = default_attribute(name, b[7], b[8])
                attr = -1 if a is None else ATTRIBUTES.index(a)
            bx = Box(f, j, gd + j, name, b, fr["det_scores"][j], attr)
            all_det.append(bx)
            if name is not None and math.hypot(float(b[0]) - ex, float(b[1]) - ey) < rng[name]:
                det.append(bx)
        kept = []
        for i in range(m):
            k = int(fr["gt_labels"][i])
            name = class_names[k] if 0 <= k < len(class_names) else None
            b = fr["gt_boxes"][i]
            if name is None or ("num_pts" in fr and int(fr["num_pts"][i]) == 0):
                continue
            if math.hypot(float(b[0]) - ex, float(b[1]) - ey) < rng[name]:
                kept.append(Box(f, i, gg + i, name, b, None, int(fr["gt_attr"][i]) if "gt_attr" in fr else -1))
        gts.append(kept)
        gd += n
        gg += m
    return all_det, det, gts, gg


def center_distance(g, d, dt):
    dx, dy = dt(g.box[0]) - dt(d.box[0]), dt(g.box[1]) - dt(d.box[1])
    return np.sqrt(dx * dx + dy * dy)


def tp_errors(g, d, dt):
    """(trans, scale, orient, vel, attr) in the arithmetic of dt."""
    gb, db = [dt(v) for v in g.box], [dt(v) for v in d.box]
    trans = center_distance(g, d, dt)
    if min(gb[3:6]) <= 0 or min(db[3:6]) <= 0:
        scale = dt(1.0)
    else:
        inter = min(gb[3], db[3]) * min(gb[4], db[4]) * min(gb[5], db[5])
        scale = dt(1.0) - inter / (gb[3] * gb[4] * gb[5] + db[3] * db[4] * db[5] - inter)
    period = dt(np.pi) if g.name == "barrier" else dt(2.0) * dt(np.pi)
    diff = (gb[6] - db[6] + period / dt(2.0)) % period - period / dt(2.0)
    if diff > dt(np.pi):
        diff = diff - dt(2.0) * dt(np.pi)
    dvx, dvy = gb[7] - db[7], gb[8] - db[8]
    vel = np.sqrt(dvx * dvx + dvy * dvy)
    attr = math.nan if g.attr < 0 else (0.0 if g.attr == d.attr else 1.0)
    return [float(trans), float(scale), float(abs(diff)), float(vel), attr]


def interp(x, xp, fp, right=None):
    """numpy.interp for non-decreasing xp, duplicates included: j is the last index with xp[j] <= x."""
    xp, fp = [float(v) for v in xp], [float(v) for v in fp]
    out = []
    for v in x:
        v = float(v)
        if v < xp[0]:
            out.append(fp[0])
        elif v > xp[-1]:
            out.append(fp[-1] if right is None else right)
        else:
            j = bisect.bisect_right(xp, v) - 1
            if j == len(xp) - 1 or xp[j] == v:
                out.append(fp[j])
            else:
                out.append((fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (v - xp[j]) + fp[j])
    return np.array(out, dtype=np.float64)


def cummean(x):
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).sum() == len(x):
        return np.ones(len(x))
    out, s, n = [], 0.0, 0
    for v in x:
        if not math.isnan(v):
            s, n = s + v, n + 1
        out.append(s / n if n else 0.0)
    return np.array(out)


def no_predictions():
    return dict(precision=np.zeros(101), confidence=np.zeros(101), **{e: np.ones(101) for e in ERRORS})


def accumulate(det, gts, name, th, dt, match_row, err_rows):
    """The devkit's accumulate for one class and threshold. match_row [n_det] / err_rows {global det: errors}
    receive the matches."""
    npos = sum(1 for kept in gts for g in kept if g.name == name)
    preds = [d for d in det if d.name == name]
    if npos == 0:
        return no_predictions()
    sortind = [i for (v, i) in sorted((float(d.score), i) for i, d in enumerate(preds))][::-1]
    tp, fp, conf, mconf, merr = [], [], [], [], []
    taken = set()
    for ind in sortind:
        d = preds[ind]
        min_dist, hit = math.inf, None
        for g in gts[d.frame]:
            if g.name == name and (g.frame, g.row) not in taken:
                dist = center_distance(g, d, dt)
                if dist < min_dist:
                    min_dist, hit = dist, g
        if hit is not None and min_dist < dt(th):
            taken.add((hit.frame, hit.row))
            tp.append(1), fp.append(0), conf.append(float(d.score))
            match_row[d.glob] = hit.glob
            e = tp_errors(hit, d, dt)
            err_rows[d.glob] = e
            mconf.append(float(d.score)), merr.append(e)
        else:
            tp.append(0), fp.append(1), conf.append(float(d.score))
    if not merr:
        return no_predictions()
    tp, fp = np.cumsum(tp).astype(float), np.cumsum(fp).astype(float)
    prec, rec = tp / (fp + tp), tp / float(npos)
    r = np.linspace(0, 1, 101)
    md = dict(precision=interp(r, rec, prec, right=0), confidence=interp(r, rec, conf, right=0))
    for k, e in enumerate(ERRORS):
        cm = cummean([row[k] for row in merr])
        md[e] = interp(md["confidence"][::-1], mconf[::-1], cm[::-1])[::-1]
    return md


def calc_ap(md, min_recall=0.1, min_precision=0.1):
    prec = np.copy(md["precision"])[round(100 * min_recall) + 1:]
    prec -= min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(md, e, min_recall=0.1):
    first = round(100 * min_recall) + 1
    nz = np.nonzero(md["confidence"])[0]
    last = 0 if len(nz) == 0 else nz[-1]
    return 1.0 if last < first else float(np.mean(md[e][first:last + 1]))


def evaluate(frames, class_names, class_range=None, thresholds=DIST_THS, dtype=np.float64, scores=True):
    """-> dict(match [T, n_det] int64, err [n_det, 5] float64 (the matches at 2.0), order [n_det], result {key:
    value} (None when scores is False), kept [n_det] bool)."""
    all_det, det, gts, n_gt = load(frames, class_names, class_range)
    n = len(all_det)
    order = np.array([i for (v, i) in sorted((float(d.score), d.glob) for d in all_det)][::-1], dtype=np.int64)
    match = np.full((len(thresholds), n), -1, dtype=np.int64)
    err = np.full((n, 5), np.nan)
    result, aps, tps = {}, [], {e: [] for e in ERRORS}
    for name in class_names:
        for t, th in enumerate(thresholds):
            rows = {}
            md = accumulate(det, gts, name, th, dtype, match[t], rows)
            if th == TP_TH:
                for j, e in rows.items():
                    err[j] = e
            if not scores:
                continue
            ap = calc_ap(md)
            aps.append(ap)
            result[f"NuScenes/{name}_AP_dist_{float(th)}"] = ap
            if th == TP_TH:
                for e in ERRORS:
                    if name == "traffic_cone" and e in ("attr", "vel", "orient"):
                        v = math.nan
                    elif name == "barrier" and e in ("attr", "vel"):
                        v = math.nan
                    else:
                        v = calc_tp(md, e)
                    result[f"NuScenes/{name}_{e}_err"] = v
                    tps[e].append(v)
    if scores:
        result["NuScenes/mAP"] = float(np.mean(aps))
        total = 5.0 * result["NuScenes/mAP"]
        for e, m in zip(ERRORS, MEANS):
            vals = [v for v in tps[e] if not math.isnan(v)]
            result[f"NuScenes/{m}"] = sum(vals) / len(vals) if vals else math.nan
            total += 1.0 - min(1.0, result[f"NuScenes/{m}"])
        result["NuScenes/NDS"] = total / 10.0
    kept = np.zeros(n, dtype=bool)
    kept[[d.glob for d in det]] = True
    gt_kept = np.zeros(n_gt, dtype=bool)
    gt_kept[[g.glob for fr in gts for g in fr]] = True
    return dict(match=match, err=err, order=order, result=result if scores else None, kept=kept, gt_kept=gt_kept)
