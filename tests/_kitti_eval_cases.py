"""Seeded inputs shared by tests/test_kitti_eval_cpu.py and tests/test_gpu_kitti_eval.py, and the comparison of
the product's intermediate results with the reference's (tests/_kitti_eval_ref.py)."""
from __future__ import annotations

import numpy as np
import torch

from tests import _kitti_eval_ref as kref
from tests import _postprocess_cases as pcs

CLASSES = ["Car", "Pedestrian", "Cyclist"]
OVERLAP_SHAPES = [(0, 7), (9, 0), (1, 1), (65, 33), (512, 128)]
TABLE_VALUES = (0.7, 0.5, 0.25)


def box(x, y, dx=4.0, dy=2.0, z=-1.0, dz=1.5, yaw=0.0):
    return [x, y, z, dx, dy, dz, yaw]


def frame(det_boxes=(), det_scores=(), det_labels=(), gt_boxes=(), gt_labels=(), det_height=None, gt_neighbor=None,
          gt_height=None, gt_occluded=None, gt_truncated=None):
    nd, ng = len(det_scores), len(gt_labels)
    f32 = np.float32

    def arr(v, n, fill, dt):
        return np.full(n, fill, dtype=dt) if v is None else np.asarray(v, dtype=dt).reshape(n)

    return dict(det_boxes=np.asarray(det_boxes, dtype=f32).reshape(nd, 7), det_scores=arr(det_scores, nd, 0, f32),
                det_labels=arr(det_labels, nd, 0, np.int64), det_height=arr(det_height, nd, np.inf, f32),
                gt_boxes=np.asarray(gt_boxes, dtype=f32).reshape(ng, 7), gt_labels=arr(gt_labels, ng, 0, np.int64),
                gt_neighbor=arr(gt_neighbor, ng, -1, np.int64), gt_height=arr(gt_height, ng, np.inf, f32),
                gt_occluded=arr(gt_occluded, ng, 0, f32), gt_truncated=arr(gt_truncated, ng, 0, f32))


def to_update(frames, device="cpu"):
    """(preds, gts) for KittiAP.update."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    preds = [dict(bboxes_3d=t(f["det_boxes"]), scores_3d=t(f["det_scores"]), labels_3d=t(f["det_labels"]),
                  bbox_height=t(f["det_height"])) for f in frames]
    gts = [dict(bboxes_3d=t(f["gt_boxes"]), labels_3d=t(f["gt_labels"]), neighbor=t(f["gt_neighbor"]),
                bbox_height=t(f["gt_height"]), occluded=t(f["gt_occluded"]), truncated=t(f["gt_truncated"]))
           for f in frames]
    return preds, gts


# ----------------------------------------------------------------------------------- hand values
def hand_single():
    """One valid ground truth matched by one detection: one threshold, precision (1, 0, ...):
    AP11 = 100 / 11, AP40 = 0."""
    return [frame([box(10, 5)], [0.8], [0], [box(10, 5)], [0])]


def hand_41():
    """41 ground truths, each matched by its own detection, distinct scores: 41 thresholds, precision 1
    everywhere: AP11 = AP40 = 100."""
    gts = [box(10.0 * k, 3.0) for k in range(41)]
    return [frame(gts, [0.95 - 0.02 * k for k in range(41)], [0] * 41, gts, [0] * 41)]


def hand_40_interleaved():
    """40 ground truths each matched, and 40 detections on nothing, interleaved in score so that every true
    positive is preceded by one higher-scored false positive: 40 thresholds, precision k / 2k = 1/2 at each,
    0 at the 41st: AP11 = 100 * 10 * 0.5 / 11 = 500 / 11, AP40 = 100 * 39 * 0.5 / 40 = 48.75."""
    gts = [box(10.0 * k, 3.0) for k in range(40)]
    dets, scores = [], []
    for k in range(40):
        dets.append(box(10.0 * k, 40.0))          # far from every ground truth
        scores.append(0.99 - 0.02 * k)
        dets.append(gts[k])
        scores.append(0.98 - 0.02 * k)
    return [frame(dets, scores, [0] * 80, gts, [0] * 40)]


# ----------------------------------------------------------------------------------- the matcher's branches
def branch_frames():
    """name -> one small frame (class 0 = Car: minimum overlap 0.7 / 0.5; an x shift s of a 4 x 2 box gives
    IoU (4 - s) / (4 + s))."""
    out = {}
    # equal scores in pass 1: detection 0 is matched (strict comparison); in the count pass detection 1 has the
    # larger overlap and takes the ground truth, detection 0 is a false positive
    out["equal_scores"] = frame([box(0.2, 0), box(0.1, 0)], [0.5, 0.5], [0, 0], [box(0, 0)], [0])
    # a Van (neighbour of Car) absorbs the detection on it: neither tp nor fp
    out["neighbour_absorbs"] = frame([box(0, 0), box(20, 0)], [0.9, 0.8], [0, 0], [box(0, 0), box(20, 0)], [-1, 0],
                                     gt_neighbor=[0, -1])
    # at the threshold 0.5 the short (flag 1) detection 0 is taken first, then displaced by the later valid
    # detection 1 (pass 1 matches detection 1: the higher score)
    out["took_ignored"] = frame([box(0.1, 0), box(0.2, 0), box(20, 0)], [0.8, 0.9, 0.5], [0, 0, 0],
                                [box(0, 0), box(20, 0)], [0, 0], det_height=[20, 60, 60], gt_height=[60, 60])
    # a short detection of ANOTHER class has flag 1, not -1: it takes ground truth 0, which is then no fn
    out["short_other_class"] = frame([box(0, 0), box(20, 0)], [0.9, 0.8], [1, 0], [box(0, 0), box(20, 0)], [0, 0],
                                     det_height=[10, 60], gt_height=[60, 60])
    # at the first threshold (0.9) the detection of score 0.3 is ignored: not a false positive, its truth a fn
    out["below_threshold"] = frame([box(0, 0), box(20, 0), box(50, 0)], [0.9, 0.3, 0.2], [0, 0, 0],
                                   [box(0, 0), box(20, 0)], [0, 0])
    # Cyclist (2) detections but no Cyclist ground truth: every Cyclist AP is 0
    out["class_without_gt"] = frame([box(0, 0), box(9, 9, 1.8, 0.6)], [0.9, 0.7], [0, 2], [box(0, 0)], [0])
    out["empty"] = frame()
    out["only_dets"] = frame([box(3, 3)], [0.4], [0])
    out["only_gts"] = frame(gt_boxes=[box(3, 3)], gt_labels=[0])
    # a hard ground truth (occluded 2, truncated 0.4, 30 px): valid for `hard` only, flag 1 for the others
    out["difficulty"] = frame([box(0, 0), box(20, 0)], [0.9, 0.8], [0, 0], [box(0, 0), box(20, 0)], [0, 0],
                              det_height=[30, 60], gt_height=[30, 60], gt_occluded=[2, 0], gt_truncated=[0.4, 0.0])
    return out


# ----------------------------------------------------------------------------------- random frames
SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])   # Car, Pedestrian, Cyclist


def random_frame(r, nd, ng, tie_scores=False):
    """ng ground truths and nd detections around one spot. About 70 % of the detections are jittered copies of
    a ground truth (so that overlaps fall on both sides of every table value), the others lie anywhere in the
    cluster. Labels, neighbours, heights, occlusion and truncation take all their kinds, so that the flags of
    both sides take all three values in every group."""
    ext = max(4.0 * np.sqrt(max(ng, 1)), 6.0)
    cx, cy = r.uniform(-60, 60, 2)
    gl = r.choice([-1, 0, 1, 2], ng, p=[0.15, 0.45, 0.2, 0.2])
    sz = SIZES[np.where(gl < 0, 0, gl)] * r.uniform(0.85, 1.2, (ng, 3))
    gb = np.stack([cx + r.uniform(0, ext, ng), cy + r.uniform(0, ext, ng), r.uniform(-2.0, -0.5, ng), sz[:, 0],
                   sz[:, 1], sz[:, 2], r.uniform(-np.pi, np.pi, ng)], 1).reshape(ng, 7)
    gn = np.where((gl < 0) & (r.rand(ng) < 0.6), r.choice([0, 1], ng), -1)
    gh = np.where(r.rand(ng) < 0.2, np.inf, r.uniform(15, 90, ng))
    go = r.choice([0, 1, 2, 3], ng, p=[0.5, 0.25, 0.15, 0.1]).astype(np.float64)
    gt = np.where(r.rand(ng) < 0.5, 0.0, r.uniform(0, 0.6, ng))
    db = np.zeros((nd, 7))
    dl = r.choice([0, 1, 2], nd)
    for j in range(nd):
        if ng and r.rand() < 0.7:
            i = r.randint(ng)
            amp = r.choice([0.03, 0.1, 0.25])
            db[j] = gb[i] + r.normal(0, 1, 7) * amp * np.array([gb[i, 3], gb[i, 4], 0.5, gb[i, 3], gb[i, 4], 0.5, 1.0])
            db[j, 3:6] = np.maximum(db[j, 3:6], 0.2)
            if gl[i] >= 0 and r.rand() < 0.85:
                dl[j] = gl[i]
        else:
            s = SIZES[dl[j]] * r.uniform(0.85, 1.2, 3)
            db[j] = [cx + r.uniform(0, ext), cy + r.uniform(0, ext), r.uniform(-2.0, -0.5), s[0], s[1], s[2],
                     r.uniform(-np.pi, np.pi)]
    ds = r.uniform(0.05, 1.0, nd)
    if tie_scores:
        ds = np.round(ds * 8) / 8
    dh = np.where(r.rand(nd) < 0.3, np.inf, r.uniform(15, 90, nd))
    return frame(db, ds, dl, gb, gl, dh, gn, gh, go, gt)


def random_frames(n, seed, cap_frame=True):
    """n seeded frames of 0 .. 40 detections and 0 .. 16 ground truths (every fourth frame with tied scores),
    plus the frame at the caps (512 detections, 128 ground truths)."""
    r = np.random.RandomState(4000 + seed)
    out = []
    for k in range(n):
        nd, ng = int(r.randint(0, 41)), int(r.randint(0, 17))
        out.append(random_frame(r, nd, ng, tie_scores=k % 4 == 3))
    if cap_frame:
        out.append(random_frame(r, 512, 128))
    return out


def drop_ambiguous(frames, margin):
    """Drop every detection that has a float64 overlap (BEV or 3D, with any ground truth of its frame) within
    `margin` of a value of either overlap table — of any class, which includes its own. -> (frames, share of
    the detections dropped, the float64 overlaps of the kept ones {mode: [per frame [nd, ng]]})."""
    out, ovs = [], {0: [], 1: []}
    total = dropped = 0
    for fr in frames:
        m = [kref.overlap_matrix(fr["det_boxes"], fr["gt_boxes"], mode) for mode in range(2)]
        bad = np.zeros(len(fr["det_scores"]), dtype=bool)
        for mm in m:
            for v in TABLE_VALUES:
                bad |= (np.abs(mm - float(np.float32(v))) < margin).any(axis=1) if mm.shape[1] else False
        total += bad.size
        dropped += int(bad.sum())
        keep = ~bad
        g = dict(fr)
        for k in ("det_boxes", "det_scores", "det_labels", "det_height"):
            g[k] = fr[k][keep]
        out.append(g)
        for mode in range(2):
            ovs[mode].append(m[mode][keep])
    return out, dropped / max(total, 1), ovs


# ----------------------------------------------------------------------------------- overlap inputs
def overlap_frames(seed=0):
    """The five frames of OVERLAP_SHAPES: boxes of 0.5 .. 5 m in a cluster small enough that about half of all
    pairs overlap, 40 .. 70 m from the origin. -> [(dets [nd, 7], gts [ng, 7])] fp32."""
    r = np.random.RandomState(5000 + seed)
    out = []
    for nd, ng in OVERLAP_SHAPES:
        cx, cy = r.uniform(40, 70) * r.choice([-1, 1]), r.uniform(40, 70) * r.choice([-1, 1])

        def boxes(n):
            return np.stack([cx + r.uniform(0, 6.0, n), cy + r.uniform(0, 6.0, n), r.uniform(-2, -0.5, n),
                             r.uniform(0.5, 5, n), r.uniform(0.5, 5, n), r.uniform(1.0, 2.5, n),
                             r.uniform(-2 * np.pi, 2 * np.pi, n)], 1).reshape(n, 7).astype(np.float32)

        out.append((boxes(nd), boxes(ng)))
    return out


def degenerate_pairs7():
    """tests/_postprocess_cases.degenerate_pairs with z = -1, dz = 1.5 on both sides, and three pairs in z.
    -> (a [n, 7], b [n, 7], expected BEV overlap or None, expected 3D overlap or None)."""
    a5, b5, want = pcs.degenerate_pairs()
    lift = lambda m: np.stack([m[:, 0], m[:, 1], np.full(len(m), -1.0), m[:, 2], m[:, 3], np.full(len(m), 1.5),
                               m[:, 4]], 1)
    a, b = lift(a5.astype(np.float64)), lift(b5.astype(np.float64))
    extra = [
        (box(10, 20, z=-1.0), box(10, 20, z=2.0), 1.0, 0.0),              # disjoint in z, the same footprint
        (box(10, 20, z=0.0, dz=1.5), box(10, 20, z=1.5, dz=1.5), 1.0, 0.0),   # touching in z
        (box(10, 20, dz=0.0), box(10, 20), 0.0, 0.0),                     # zero height: no box in either mode
        (box(-70, 65, 3.9, 1.6, -1.7, 1.56, 1.57), box(-70, 65, 3.9, 1.6, -1.7, 1.56, 1.57), 1.0, 1.0),
    ]
    a = np.concatenate([a, np.asarray([e[0] for e in extra])]).astype(np.float32)
    b = np.concatenate([b, np.asarray([e[1] for e in extra])]).astype(np.float32)
    return a, b, list(want) + [e[2] for e in extra], list(want) + [e[3] for e in extra]


def extreme_pairs7():
    big = 3e38
    a = [[0, 0, 0, big, big, big, 0], [big, -big, big, 1, 1, 1, 1e30], [0, 0, 0, 1e-30, 1e-30, 1e-30, 0],
         [1e20, 1e20, -1e20, 1e19, 1, 1e19, 3], [0, 0, -big, 1, 1, big, 0]]
    b = [[0, 0, 0, big, big, big, 1], [-big, big, -big, big, 1, big, -1e30], [0, 0, 0, 1e-30, 1e-30, 1e-30, 0],
         [1e20, 1e20, 1e20, 1, 1e19, 1, 2], [0, 0, big, 1, 1, big, 0]]
    return np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)


# ----------------------------------------------------------------------------------- comparison
def product_detail(metric, overlaps=None):
    """Run the metric's counting with its intermediate results exposed."""
    detail = {}
    counts, nthr = metric._counts(overlaps=overlaps, detail=detail)
    return counts, nthr, detail


def frame_overlaps(detail):
    """The product's overlap matrices as the reference takes them: {mode: [per frame [nd, ng] numpy]}."""
    d_off, g_off, o_off = detail["det_off"], detail["gt_off"], detail["ov_off"]
    out = {}
    for mode in range(2):
        ov = detail["overlaps"][mode].cpu().numpy()
        out[mode] = [ov[o_off[f]:o_off[f + 1]].reshape(d_off[f + 1] - d_off[f], g_off[f + 1] - g_off[f])
                     for f in range(len(d_off) - 1)]
    return out


def assert_equal_to_reference(counts, nthr, detail, want, n_classes=3):
    """Pass-1 scores, thresholds and every tp / fp / fn of every group equal the reference's, no tolerance."""
    G = n_classes * 6
    tps = detail["tp_scores"].cpu().numpy()
    thr = detail["thr"].cpu().numpy()
    g_off = detail["gt_off"]
    counts = counts.numpy()
    for (mode, c, d, t), w in want.items():
        g = (c * 3 + d) * 2 + t
        q = mode * G + g
        exp = np.full(g_off[-1], float(kref.NO))
        for f, em in enumerate(w["tp_scores"]):
            for i, s in em:
                exp[g_off[f] + i] = s
        assert np.array_equal(tps[mode, g].astype(np.float64), exp), (mode, c, d, t)
        assert detail["n_valid_gt"][c * 3 + d] == w["n_valid_gt"]
        assert nthr[q] == len(w["thresholds"]), (mode, c, d, t, nthr[q], len(w["thresholds"]))
        assert thr[mode, g, :nthr[q]].astype(np.float64).tolist() == w["thresholds"], (mode, c, d, t)
        assert [tuple(v) for v in counts[q, :nthr[q]].tolist()] == w["counts"], (mode, c, d, t)
        assert not counts[q, nthr[q]:].any()
