"""Inputs of the nuScenes detection score tests, built so that float32 takes float64's decisions: xy on the 1/8 m
grid within +-54 m (dx^2 + dy^2 is then exact in fp32, and objects fall on both sides of every class range), scores
on a 1/64 grid (ties occur), dims / yaw / velocities arbitrary float32 with yaw over [-2 pi, 2 pi]. Frames are the
dicts of tests/_nuscenes_eval_ref.py."""
import numpy as np
import torch

CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
           "traffic_cone"]
CAR, TRUCK, CV, BUS, TRAILER, BARRIER, MOTO, BICYCLE, PED, CONE = range(10)
SHAPES = [(0, 5), (7, 0), (1, 1), (65, 33), (500, 512)]
EIGHT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0, 0.25, 8.0, 3.0, 1.5)     # every square exact in fp32
F02 = float(np.float32(0.2))


def _frame(dets, gts, **extra):
    """dets: (x, y, label, score[, dict(yaw, vx, vy, dims, attr)]); gts: (x, y, label[, dict(yaw, vx, vy, dims,
    attr, num_pts)])."""
    def boxes(rows, k0):
        out = np.zeros((len(rows), 9), np.float32)
        for r, row in enumerate(rows):
            o = row[k0] if len(row) > k0 else {}
            out[r, :2] = row[0], row[1]
            out[r, 2] = -1.0
            out[r, 3:6] = o.get("dims", (2.0, 4.0, 1.5))
            out[r, 6], out[r, 7], out[r, 8] = o.get("yaw", 0.25), o.get("vx", 0.0), o.get("vy", 0.0)
        return out

    fr = dict(det_boxes=boxes(dets, 4), det_scores=np.array([d[3] for d in dets], np.float32),
              det_labels=np.array([d[2] for d in dets], np.int64), gt_boxes=boxes(gts, 3),
              gt_labels=np.array([g[2] for g in gts], np.int64))
    opt = lambda rows, k0, key, fill: np.array([(r[k0] if len(r) > k0 else {}).get(key, fill) for r in rows], np.int64)
    if any("attr" in (g[3] if len(g) > 3 else {}) for g in gts):
        fr["gt_attr"] = opt(gts, 3, "attr", -1)
    if any("num_pts" in (g[3] if len(g) > 3 else {}) for g in gts):
        fr["num_pts"] = opt(gts, 3, "num_pts", 5)
    if any("attr" in (d[4] if len(d) > 4 else {}) for d in dets):
        fr["det_attr"] = opt(dets, 4, "attr", -1)
    fr.update(extra)
    return fr


def branch_frames():
    """One frame per rule of the specification. In this set alone: trailer has ground truth and no match,
    construction_vehicle has detections and no ground truth, bicycle's recall stays below 0.1."""
    pi = float(np.pi)
    f = {}
    # two detections contend for one ground truth: the loser is fp up to t = 2 and takes the farther one at t = 4
    f["contend"] = _frame([(0.125, 0, CAR, 0.875), (0.25, 0, CAR, 0.5)], [(0, 0, CAR), (3, 0, CAR)])
    # the nearest ground truth is taken, the second nearest (0.75 m) is within t = 1
    f["second_nearest"] = _frame([(10, 0, CAR, 0.875), (10.25, 0, CAR, 0.5)], [(10, 0, CAR), (11, 0, CAR)])
    # a distance exactly equal to each threshold is no match at it
    f["exact_threshold"] = _frame([(0.5, 0, TRUCK, 0.75), (21, 0, TRUCK, 0.625), (-22, 0, TRUCK, 0.5), (0, 24, TRUCK, 0.375)],
                                  [(0, 0, TRUCK), (20, 0, TRUCK), (-20, 0, TRUCK), (0, 20, TRUCK)])
    # two (three) equidistant ground truths: the lowest row wins
    f["equidistant"] = _frame([(0, 0, BUS, 0.75), (20, 20, BUS, 0.5)],
                              [(0, -1, BUS), (0, 1, BUS), (20, 21, BUS), (21, 20, BUS), (20, 19, BUS)])
    # equal scores: the later row goes first and takes the ground truth although the earlier one is nearer
    f["equal_scores"] = _frame([(0, 0.125, PED, 0.5), (0, 0.25, PED, 0.5), (8, 8, PED, 0.5)], [(0, 0, PED), (8, 8.125, PED)])
    # a nearer ground truth of another class is ignored
    f["other_class"] = _frame([(5, 5, CAR, 0.625)], [(5, 5.125, PED), (5, 5.375, CAR), (5, 5, -1)])
    # a class with ground truth and no match; a class with detections and no ground truth
    f["no_match"] = _frame([(-10, -10, TRAILER, 0.75), (3, 3, CV, 0.5)], [(10, 10, TRAILER)])
    # exactly at the class range: dropped (strict <); one grid step inside: kept
    f["range"] = _frame([(30, 40, CAR, 0.875), (30, 39.875, CAR, 0.75), (24, 32, PED, 0.625), (24, 31.875, PED, 0.5),
                         (18, 24, CONE, 0.375), (18, 23.875, CONE, 0.25), (-18, -24, BARRIER, 0.25),
                         (-18, -23.875, BARRIER, 0.125)],
                        [(30, 40, CAR), (30, 39.875, CAR), (24, 32, PED), (24, 31.875, PED), (18, 24, CONE),
                         (18, 23.875, CONE), (-18, -24, BARRIER), (-18, -23.875, BARRIER)])
    # a ground truth without lidar points is dropped: the detection on it is a false positive
    f["num_pts"] = _frame([(-30, 0, CAR, 0.75), (-30, 8, CAR, 0.5)], [(-30, 0, CAR, dict(num_pts=0)), (-30, 8, CAR, dict(num_pts=3))])
    # recall 1 / 11 < 0.1: AP 0 and every error 1
    f["low_recall"] = _frame([(0, -30, BICYCLE, 0.5)], [(2 * k - 10, -30, BICYCLE) for k in range(11)])
    # yaw: a barrier pair pi apart has error 0, a car pair pi; the wraps of [-2 pi, 2 pi]
    f["yaw"] = _frame([(-5, 20, BARRIER, 0.75, dict(yaw=0.5 + pi)), (5, 20, CAR, 0.75, dict(yaw=0.5 + pi)),
                       (15, 20, CAR, 0.5, dict(yaw=-2 * pi + 0.125)), (25, 20, CAR, 0.5, dict(yaw=1.75 * pi)),
                       (-15, 20, BARRIER, 0.5, dict(yaw=-1.875 * pi)), (-20, 20, BARRIER, 0.25, dict(yaw=0.75))],
                      [(-5, 20, BARRIER, dict(yaw=0.5)), (5, 20, CAR, dict(yaw=0.5)), (15, 20, CAR, dict(yaw=2 * pi - 0.25)),
                       (25, 20, CAR, dict(yaw=-1.75 * pi)), (-15, 20, BARRIER, dict(yaw=1.75 * pi)),
                       (-20, 20, BARRIER, dict(yaw=0.75 + pi / 2))])
    # attributes: a ground truth with none (-1: NaN), and the speed-0.2 boundary of the rule per class group
    still, moving = dict(vx=0.125, vy=0.125), dict(vx=0.25, vy=0.0)
    edge = dict(vx=F02, vy=0.0)      # float32(0.2) > 0.2: moving
    f["attributes"] = _frame(
        [(0, 10, CAR, 0.75, still), (4, 10, CAR, 0.75, moving), (8, 10, CAR, 0.625, edge), (12, 10, BUS, 0.5, still),
         (16, 10, BUS, 0.5, moving), (20, 10, PED, 0.5, still), (24, 10, PED, 0.5, moving), (28, 10, MOTO, 0.5, still),
         (32, 10, MOTO, 0.375, moving), (0, 14, TRUCK, 0.375, moving), (4, 14, CONE, 0.5, moving),
         (8, 14, BARRIER, 0.5, still), (12, 14, CAR, 0.25, still), (16, 14, TRUCK, 0.25, edge)],
        [(0, 10, CAR, dict(attr=6)), (4, 10, CAR, dict(attr=5)), (8, 10, CAR, dict(attr=5)), (12, 10, BUS, dict(attr=7)),
         (16, 10, BUS, dict(attr=7)), (20, 10, PED, dict(attr=3)), (24, 10, PED, dict(attr=3)), (28, 10, MOTO, dict(attr=1)),
         (32, 10, MOTO, dict(attr=1)), (0, 14, TRUCK, dict(attr=5)), (4, 14, CONE, dict(attr=-1)),
         (8, 14, BARRIER, dict(attr=-1)), (12, 14, CAR, dict(attr=-1)), (16, 14, TRUCK, dict(attr=6))])
    # detections that carry their own attributes
    f["det_attributes"] = _frame([(0, -10, CAR, 0.75, dict(attr=7, vx=3.0)), (4, -10, PED, 0.5, dict(attr=4))],
                                 [(0, -10, CAR, dict(attr=7)), (4, -10, PED, dict(attr=2))])
    # a non-zero ego origin: (40, 35) is 50 m from it (dropped), one step nearer is kept; from (0, 0) both are outside
    f["ego_origin"] = _frame([(40, 35, CAR, 0.75), (40, 34.875, CAR, 0.5)], [(40, 35, CAR), (40, 34.875, CAR)],
                             ego=(10.0, -5.0))
    # an extent of 0 gives scale error 1; a NaN ground-truth velocity gives a NaN velocity error
    f["degenerate"] = _frame([(-35, 0, MOTO, 0.75), (-35, 8, MOTO, 0.5, dict(dims=(1.0, 0.0, 1.0))), (-35, 16, MOTO, 0.25)],
                             [(-35, 0, MOTO, dict(dims=(0.0, 2.0, 1.0))), (-35, 8, MOTO), (-35, 16, MOTO, dict(vx=float("nan")))])
    return f


def _random_frame(rng, nd, ng):
    grid = lambda n: rng.integers(-54 * 8, 54 * 8 + 1, (n, 2)) / 8.0
    gt = np.zeros((ng, 9), np.float32)
    gt[:, :2] = grid(ng)
    gl = rng.integers(0, 10, ng)
    gl[rng.random(ng) < 0.03] = -1
    det = np.zeros((nd, 9), np.float32)
    dl = rng.integers(0, 10, nd)
    xy = grid(nd)
    if ng:
        src = rng.permutation(max(nd, ng))[:nd] % ng       # contention, but spread over the ground truths
        near = rng.random(nd) < 0.8
        spread = rng.choice([2, 8, 24], nd, p=[0.5, 0.3, 0.2])[:, None]      # grid steps: 0.25, 1, 3 m
        off = rng.integers(-spread, spread + 1, (nd, 2)) / 8.0
        xy = np.where(near[:, None], np.clip(gt[src, :2] + off, -54, 54), xy)
        dl = np.where(near & (gl[src] >= 0), gl[src], dl)
    det[:, :2] = xy
    for b in (det, gt):
        n = len(b)
        b[:, 2] = rng.uniform(-3, 1, n)
        b[:, 3:6] = rng.uniform(0.3, 6.0, (n, 3))
        b[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, n)
        b[:, 7:9] = rng.normal(0, 1.5, (n, 2))
    det[rng.random(nd) < 0.3, 7:9] *= 0.05        # slow detections: the attribute rule's other side
    gt[rng.random(ng) < 0.05, 7] = np.nan
    return dict(det_boxes=det, det_scores=(rng.integers(1, 65, nd) / 64.0).astype(np.float32), det_labels=dl.astype(np.int64),
                gt_boxes=gt, gt_labels=gl.astype(np.int64), gt_attr=rng.integers(-1, 8, ng).astype(np.int64),
                num_pts=np.where(rng.random(ng) < 0.05, 0, rng.integers(1, 50, ng)).astype(np.int64))


def random_frames(n, seed):
    """n frames over the ten classes with (Nd, Ng) up to (120, 60)."""
    rng = np.random.default_rng(seed)
    return [_random_frame(rng, int(rng.integers(20, 121)), int(rng.integers(10, 61))) for _ in range(n)]


def shape_frames(seed=1):
    """The empty sides, one pair, a wave boundary, and the frame at the caps (500 detections, 512 ground truths)."""
    rng = np.random.default_rng(seed)
    return [_random_frame(rng, nd, ng) for nd, ng in SHAPES]


def to_update(frames, device=None):
    """-> (preds, gts) for NuScenesDetectionScore.update; detections on `device`."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    d = (lambda a: t(a).to(device)) if device is not None else t
    preds, gts = [], []
    for fr in frames:
        p = dict(bboxes_3d=d(fr["det_boxes"]), scores_3d=d(fr["det_scores"]), labels_3d=d(fr["det_labels"]))
        if "det_attr" in fr:
            p["attr_labels"] = d(fr["det_attr"])
        g = dict(bboxes_3d=t(fr["gt_boxes"]), labels_3d=t(fr["gt_labels"]))
        if "gt_attr" in fr:
            g["attr_labels"] = t(fr["gt_attr"])
        if "num_pts" in fr:
            g["num_pts"] = t(fr["num_pts"])
        if "ego" in fr:
            g["ego_origin"] = fr["ego"]
        preds.append(p)
        gts.append(g)
    return preds, gts


def flat_inputs(frames, ref):
    """The flat arrays `center_matches` takes, from the frames and the reference's evaluation (its order and keep
    flags): the detections in evaluation order inside each frame. -> dict of numpy arrays and `perm`, the global
    detection index of every row."""
    nd = [len(fr["det_boxes"]) for fr in frames]
    frame = np.repeat(np.arange(len(frames)), nd)
    order = ref["order"]
    perm = order[np.argsort(frame[order], kind="stable")]
    det = np.concatenate([fr["det_boxes"] for fr in frames])
    gt = np.concatenate([fr["gt_boxes"] for fr in frames])
    return dict(det_xy=det[perm, :2], det_label=np.concatenate([fr["det_labels"] for fr in frames])[perm],
                det_keep=ref["kept"][perm], det_off=np.cumsum([0] + nd).tolist(), gt_xy=gt[:, :2],
                gt_label=np.concatenate([fr["gt_labels"] for fr in frames]), gt_keep=ref["gt_kept"],
                gt_off=np.cumsum([0] + [len(fr["gt_boxes"]) for fr in frames]).tolist(), perm=perm)
