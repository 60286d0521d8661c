"""Seeded inputs shared by tests/test_kitti_calib_cpu.py and tests/test_gpu_kitti_calib.py for the calibration
side of the KITTI evaluator, and the conditions that keep every decision out of rounding noise. Every condition is
checked with the reference alone (tests/_kitti_calib_ref.py: float64 against its own float32 restatement), on the
CPU; boxes that violate one are removed here, on the host, before the product or the reference sees them, and at
most 2 % of a case may go.

  every corner has |W| >= 0.05 m (some boxes straddle the camera plane: corners of negative W);
  raw box edges are >= 1e-2 px from the four validity comparisons;
  clipped heights are >= 1e-2 px from 25 and 40;
  bottom centres are >= 1e-3 m from the faces of pcd_limit_range;
  2D overlaps and DontCare ratios are further from a minimum overlap than the measured overlap bound.
Each pixel margin is widened to 4 x the float32 restatement's own error on that very box where that is larger (a
corner at W = 0.05 m magnifies the fp32 rounding of W by 20 / m), and the overlap margin likewise to 4 x the change
of that overlap when the boxes come from the float32 projection.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import _kitti_calib_ref as cref
from tests import _kitti_eval_cases as cs
from tests import _kitti_eval_ref as kref

CLASSES = cs.CLASSES
IMG_HW = (375, 1242)
RANGE = cref.PCD_LIMIT_RANGE
STRICT_VALUES = (0.7, 0.5)          # the minimum overlaps of the 2D / AOS metrics and of the DontCare test
MIN_W, PX, METRE, MAX_SHARE = 0.05, 1e-2, 1e-3, 0.02
PROJECT_COUNTS = [0, 1, 255, 257, 513]
DC_COUNTS = [0, 1, 64]


# ----------------------------------------------------------------------------------- calibration
def calibration(k=0):
    """A KITTI-like calibration, distinct for every k: fx = fy = 721.5377, the usual axis permutation in
    Tr_velo_to_cam with a small rotation, a near-identity R0_rect. -> (P2, R0_rect, Tr_velo_to_cam) float64."""
    r = np.random.RandomState(7000 + k)
    P2 = np.array([[721.5377, 0.0, 609.5593 + 2.0 * k, 44.85728], [0.0, 721.5377, 172.854 - 1.5 * k, 0.2163791],
                   [0.0, 0.0, 1.0, 0.002745884]])

    def rot(ax, ay, az):
        cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
        return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))

    R0 = rot(*r.uniform(-0.01, 0.01, 3))
    perm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    Tr = np.concatenate([rot(*r.uniform(-0.01, 0.01, 3)) @ perm,
                         np.array([[-0.004], [-0.076], [-0.272]]) + r.uniform(-0.01, 0.01, (3, 1))], 1)
    return P2, R0, Tr


def matrix(k=0):
    return cref.lidar2img(*calibration(k))


def identity_like():
    """x forward is the depth, u = 100 y + 500 W, v = 100 z + 200 W: u = 500 + 100 y / x, v = 200 + 100 z / x."""
    return np.array([[500.0, 100.0, 0.0, 0.0], [200.0, 0.0, 100.0, 0.0], [1.0, 0.0, 0.0, 0.0]], dtype=np.float32)


# ----------------------------------------------------------------------------------- per-box conditions
def box_conditions(boxes, mats, hws, check_valid=True, check_height=True):
    """-> bad [n] bool (a condition of the module docstring fails; a NaN box is exempt: it is invalid whatever
    the rounding), the float64 projections and the float32 restatement."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 7)
    n = len(boxes)
    mats = np.broadcast_to(np.asarray(mats, dtype=np.float32).reshape(-1, 12), (n, 12))
    hws = np.broadcast_to(np.asarray(hws, dtype=np.float32).reshape(-1, 2), (n, 2))
    p64 = [cref.project(boxes[k], mats[k], hws[k], RANGE) for k in range(n)]
    p32 = cref.project_f32(boxes, mats, hws) if n else None
    bad = np.zeros(n, dtype=bool)
    for k, p in enumerate(p64):
        if not np.isfinite(boxes[k]).all():
            continue
        h, w = float(hws[k][0]), float(hws[k][1])
        if min(abs(v) for v in p["w"]) < MIN_W:
            bad[k] = True
            continue
        e = np.abs(p32["raw"][k].astype(np.float64) - np.array(p["raw"]))
        if not np.isfinite(e).all():
            bad[k] = True
            continue
        if check_valid:
            for v, lim, err in ((p["raw"][0], w, e[0]), (p["raw"][1], h, e[1]), (p["raw"][2], 0.0, e[2]),
                                (p["raw"][3], 0.0, e[3])):
                bad[k] |= abs(v - lim) < max(PX, 4.0 * err)
            for a, face in zip((0, 1, 2, 0, 1, 2), RANGE):
                bad[k] |= abs(float(boxes[k][a]) - face) < METRE
        if check_height:
            eh = abs(float(p32["height"][k]) - p["height"])
            for lim in (25.0, 40.0):
                bad[k] |= abs(p["height"] - lim) < max(PX, 4.0 * eh)
    return bad, p64, p32


def _random_boxes(r, n, near=0.15):
    """Boxes in front of, beside, below and across the camera: about `near` of them within a box length of the
    camera plane (corners of negative W), a few outside pcd_limit_range and outside the image."""
    x = np.where(r.rand(n) < near, r.uniform(-1.5, 3.0, n), r.uniform(3.0, 78.0, n))
    y = r.uniform(-1.1, 1.1, n) * np.maximum(x, 4.0) * 0.9
    y = np.where(r.rand(n) < 0.1, r.uniform(-45, 45, n), y)
    z = np.where(r.rand(n) < 0.1, r.uniform(-4.0, 0.8, n), r.uniform(-2.6, -0.4, n))
    return np.stack([x, y, z, r.uniform(0.4, 5.0, n), r.uniform(0.4, 2.5, n), r.uniform(1.0, 2.5, n),
                     r.uniform(-2 * np.pi, 2 * np.pi, n)], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def project_case():
    """F = 5 frames of PROJECT_COUNTS boxes, a distinct matrix and image size per frame, and 3 rows past the last
    offset. -> dict(boxes [n + 3, 7], off, mats [5, 12], hws [5, 2], p64 (per row of a frame), p32, share)."""
    r = np.random.RandomState(7100)
    frames, tried, gone = [], 0, 0
    mats = np.stack([matrix(k).reshape(-1) for k in range(5)])
    hws = np.array([[375, 1242], [370, 1224], [376, 1241], [374, 1238], [375, 1242]], dtype=np.float32)
    for f, cnt in enumerate(PROJECT_COUNTS):
        cand = _random_boxes(r, cnt + 24)
        bad = box_conditions(cand, mats[f], hws[f])[0]
        good = cand[~bad][:cnt]
        assert len(good) == cnt
        used = int(np.searchsorted(np.cumsum(~bad), cnt)) + 1 if cnt else 0
        tried += used
        gone += int(bad[:used].sum())
        frames.append(good)
    frames[3][7] = np.nan                      # a NaN box and a box whose yaw alone is NaN: invalid
    frames[3][8, 6] = np.nan
    off = np.cumsum([0] + PROJECT_COUNTS).tolist()
    boxes = np.concatenate(frames + [_random_boxes(r, 3)])
    rows = np.repeat(np.arange(5), PROJECT_COUNTS)
    _, p64, p32 = box_conditions(boxes[:off[-1]], mats[rows], hws[rows])
    return dict(boxes=boxes, off=off, mats=mats, hws=hws, rows=rows, p64=p64, p32=p32, share=gone / max(tried, 1))


# ----------------------------------------------------------------------------------- 2D overlaps
def boxes_2d(r, n, spread=300.0):
    x1, y1 = r.uniform(200, 200 + spread, n), r.uniform(100, 100 + spread / 2, n)
    return np.stack([x1, y1, x1 + r.uniform(20, 250, n), y1 + r.uniform(20, 150, n)], 1).astype(np.float32)


def degenerate_2d():
    """(det, gt, expected IoU or None): identical, touching, zero area, negative side, slivers, shared edges."""
    rows = [
        ([10, 20, 110, 70], [10, 20, 110, 70], 1.0),            # identical
        ([10, 20, 110, 70], [110, 20, 210, 70], 0.0),           # touching at an edge
        ([10, 20, 110, 70], [110, 70, 210, 170], 0.0),          # touching at a corner
        ([10, 20, 10, 70], [0, 0, 100, 100], 0.0),              # zero width
        ([10, 20, 110, 20], [0, 0, 100, 100], 0.0),             # zero height
        ([110, 20, 10, 70], [0, 0, 200, 100], 0.0),             # negative width
        ([0, 0, 100, 100], [50, 50, 50, 60], 0.0),              # zero-area ground truth
        ([0, 0, 100, 100], [99.999, 0, 200, 100], None),        # a 1e-3 px sliver
        ([0, 0, 100, 1e-3], [0, 0, 100, 1e-3], 1.0),            # a sliver against itself
        ([0, 0, 100, 100], [0, 0, 100, 50], 0.5),               # shared edges, half
        ([0, 0, 100, 100], [0, 0, 50, 50], 0.25),
        ([0, 0, 1242, 375], [100, 100, 101, 101], None),
        ([0, 0, 0, 0], [0, 0, 0, 0], 0.0),                      # the clipped box of a NaN projection
    ]
    return (np.array([r[0] for r in rows], dtype=np.float32), np.array([r[1] for r in rows], dtype=np.float32),
            [r[2] for r in rows])


@functools.lru_cache(maxsize=None)
def overlap2d_case():
    """The frames of cs.OVERLAP_SHAPES in 2D, then one frame of one pair per row of the degenerate table. ->
    dict(dets, det_off, gts, gt_off, f64, f32 flat in the product's order, n5, wants)."""
    r = np.random.RandomState(7200)
    frames = [(boxes_2d(r, nd), boxes_2d(r, ng)) for nd, ng in cs.OVERLAP_SHAPES]
    d, g, wants = degenerate_2d()
    frames += [(d[k:k + 1], g[k:k + 1]) for k in range(len(d))]
    det_off = np.cumsum([0] + [len(a) for a, _ in frames]).tolist()
    gt_off = np.cumsum([0] + [len(b) for _, b in frames]).tolist()
    f64 = np.concatenate([cref.iou_matrix(a, b).reshape(-1) for a, b in frames])
    f32 = np.concatenate([cref.iou_matrix_f32(a, b).reshape(-1) for a, b in frames])
    n5 = sum(len(a) * len(b) for a, b in frames[:5])
    return dict(dets=np.concatenate([a for a, _ in frames]), det_off=det_off, gts=np.concatenate([b for _, b in frames]),
                gt_off=gt_off, f64=f64, f32=f32, n5=n5, wants=wants)


@functools.lru_cache(maxsize=None)
def dc_case():
    """Frames of 40 detections against DC_COUNTS DontCare boxes. The ratio bound is measured like the overlap
    bound; detections whose largest ratio is within it of a strict value are removed. -> dict(dets, det_off, dcs,
    dc_off, want [2][n] for STRICT_VALUES, ref_err, share)."""
    r = np.random.RandomState(7300)
    raw = [(boxes_2d(r, 40), boxes_2d(r, k)) for k in DC_COUNTS]
    r64 = [cref.dc_matrix(a, b) for a, b in raw]
    r32 = [cref.dc_matrix_f32(a, b) for a, b in raw]
    ref_err = max([float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(r32, r64) if y.size] + [0.0])
    frames, want, total, gone = [], [], 0, 0
    for (a, b), m in zip(raw, r64):
        best = m.max(1) if m.shape[1] else np.zeros(len(a))
        bad = np.zeros(len(a), dtype=bool)
        for v in STRICT_VALUES:
            bad |= np.abs(best - float(np.float32(v))) < 4.0 * ref_err
        total, gone = total + len(a), gone + int(bad.sum())
        frames.append((a[~bad], b))
        want.append(np.stack([best[~bad] > float(np.float32(v)) for v in STRICT_VALUES]))
    det_off = np.cumsum([0] + [len(a) for a, _ in frames]).tolist()
    dc_off = np.cumsum([0] + [len(b) for _, b in frames]).tolist()
    return dict(dets=np.concatenate([a for a, _ in frames]), det_off=det_off, dcs=np.concatenate([b for _, b in frames]),
                dc_off=dc_off, want=np.concatenate(want, 1), ref_err=ref_err, share=gone / total)


@functools.lru_cache(maxsize=None)
def overlap_bound_2d():
    """4 x the float32 restatement's own maximum error against float64 on overlap2d_case: the bound of the GPU
    overlap test and the margin of the 2D overlaps here."""
    c = overlap2d_case()
    return 4.0 * float(np.abs(c["f32"].astype(np.float64) - c["f64"]).max())


@functools.lru_cache(maxsize=None)
def overlap_bound_3d():
    """The bound of tests/test_gpu_kitti_eval.py::test_box_overlaps, the larger of its two modes."""
    frames = cs.overlap_frames()
    a, b, _, _ = cs.degenerate_pairs7()
    frames += [(b[k:k + 1], a[k:k + 1]) for k in range(len(a))]
    err = 0.0
    for mode in range(2):
        for d, g in frames:
            if len(d) and len(g):
                err = max(err, float(np.abs(kref.overlap_matrix(d, g, mode, np.float32).astype(np.float64)
                                            - kref.overlap_matrix(d, g, mode, np.float64)).max()))
    return 4.0 * err


# ----------------------------------------------------------------------------------- whole frames
def calib_frame(r, k, nd, ng, n_dc=None, near=False, tie_scores=False):
    """cs.random_frame moved in front of the camera of calibration k (near: across the camera plane), with the
    calibration fields. Every other frame leaves the ground truths' heights to the projection, every third gives
    annotated 2D boxes, every fourth annotated angles, every second has DontCare regions."""
    fr = cs.random_frame(r, nd, ng, tie_scores)
    xs = np.concatenate([fr["det_boxes"][:, 0], fr["gt_boxes"][:, 0], [0.0]])
    ys = np.concatenate([fr["det_boxes"][:, 1], fr["gt_boxes"][:, 1], [0.0]])
    tx = r.uniform(-2.5, 1.0) if near else r.uniform(4.0, 45.0)
    ty = r.uniform(-0.5, -0.1) * (ys.max() - ys.min())
    for key in ("det_boxes", "gt_boxes"):
        fr[key] = fr[key].copy()
        fr[key][:, 0] += np.float32(tx - xs[:-1].min() if len(xs) > 1 else 0.0)
        fr[key][:, 1] += np.float32(ty - ys[:-1].min() if len(ys) > 1 else 0.0)
    low = r.rand(nd) < 0.05
    fr["det_boxes"][low, 2] -= np.float32(1.6)              # some detections below the range
    fr["lidar2img"], fr["img_shape"] = matrix(k), IMG_HW
    mat, hw = fr["lidar2img"].reshape(-1), np.array(IMG_HW, dtype=np.float32)
    if k % 2 == 1:
        fr["gt_height_given"] = False
    if ng and k % 3 == 0:
        clip = cref.project_f32(fr["gt_boxes"], np.tile(mat, (ng, 1)), np.tile(hw, (ng, 1)))["clip"]
        fr["gt_bbox"] = (clip + r.uniform(-3, 3, clip.shape)).astype(np.float32)
    if ng and k % 4 == 0:
        fr["gt_alpha"] = r.uniform(-np.pi, np.pi, ng)
    if n_dc is None:
        n_dc = int(r.randint(0, 6)) if k % 2 == 0 else 0
    if n_dc:
        x1, y1 = r.uniform(0, 1100, n_dc), r.uniform(0, 300, n_dc)
        fr["dontcare"] = np.stack([x1, y1, x1 + r.uniform(40, 300, n_dc), y1 + r.uniform(30, 120, n_dc)],
                                  1).astype(np.float32)
    return fr


def filter_frame(fr, m2d, m3d):
    """Remove the detections and ground truths that violate a condition. -> (frame, boxes looked at, removed)."""
    nd, ng = len(fr["det_scores"]), len(fr["gt_labels"])
    mat, hw = fr["lidar2img"].reshape(-1), np.array(fr["img_shape"], dtype=np.float32)
    bad_g = box_conditions(fr["gt_boxes"], mat, hw, check_valid=False,
                           check_height=not fr.get("gt_height_given", True))[0]
    bad_g |= ~np.isfinite(fr["gt_boxes"]).all(1)
    g = dict(fr)
    for key in ("gt_boxes", "gt_labels", "gt_neighbor", "gt_height", "gt_occluded", "gt_truncated", "gt_bbox",
                "gt_alpha"):
        if key in fr:
            g[key] = fr[key][~bad_g]
    bad_d, p64, p32 = box_conditions(fr["det_boxes"], mat, hw)
    bad_d |= ~np.isfinite(fr["det_boxes"]).all(1)
    # 2D overlaps and DontCare ratios, in float64 and from the float32 restatement's boxes
    ngk = len(g["gt_labels"])
    if nd:
        d64 = np.array([p["clip"] for p in p64]).reshape(nd, 4)
        d32 = p32["clip"]
        if ngk:
            gm, ghw = np.tile(mat, (ngk, 1)), np.tile(hw, (ngk, 1))
            g64 = np.asarray(g["gt_bbox"], dtype=np.float64) if "gt_bbox" in g else np.array(
                [cref.project(b, mat, hw)["clip"] for b in g["gt_boxes"]]).reshape(ngk, 4)
            g32 = g["gt_bbox"] if "gt_bbox" in g else cref.project_f32(g["gt_boxes"], gm, ghw)["clip"]
            a, b = cref.iou_matrix(d64, g64), cref.iou_matrix_f32(d32, g32).astype(np.float64)
            for v in STRICT_VALUES:
                bad_d |= (np.abs(a - float(np.float32(v))) < np.maximum(m2d, 4.0 * np.abs(a - b))).any(1)
        if "dontcare" in fr:
            a = cref.dc_matrix(d64, fr["dontcare"]).max(1)
            b = cref.dc_matrix_f32(d32, fr["dontcare"]).astype(np.float64).max(1)
            for v in STRICT_VALUES:
                bad_d |= np.abs(a - float(np.float32(v))) < np.maximum(m2d, 4.0 * np.abs(a - b))
    for key in ("det_boxes", "det_scores", "det_labels", "det_height"):
        g[key] = fr[key][~bad_d]
    (g,), _, _ = cs.drop_ambiguous([g], m3d)                # the BEV / 3D overlaps, as the evaluator's tests do
    removed = int(bad_g.sum()) + nd - len(g["det_scores"])
    return g, nd + ng, removed


@functools.lru_cache(maxsize=None)
def eval_frames(n=36, seed=0):
    """About 40 calibrated frames, filtered: n random ones (every sixth across the camera plane), and the frame at
    the caps (512 detections, 128 ground truths, 64 DontCare boxes). -> (frames, share removed)."""
    r = np.random.RandomState(7400 + seed)
    m2d, m3d = overlap_bound_2d(), overlap_bound_3d()
    out, total, gone = [], 0, 0
    for k in range(n + 1):
        if k < n:
            fr = calib_frame(r, k, int(r.randint(0, 41)), int(r.randint(0, 17)), near=k % 6 == 5, tie_scores=k % 4 == 3)
        else:
            fr = calib_frame(r, k, 512, 128, n_dc=64)
        fr, looked, removed = filter_frame(fr, m2d, m3d)
        out.append(fr)
        total, gone = total + looked, gone + removed
    return out, gone / max(total, 1)


def to_update(frames, device="cpu", with_height=True):
    """(preds, gts) for KittiAP.update, with the calibration fields."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    preds, gts = [], []
    for f in frames:
        p = dict(bboxes_3d=t(f["det_boxes"]), scores_3d=t(f["det_scores"]), labels_3d=t(f["det_labels"]))
        if with_height:
            p["bbox_height"] = t(f["det_height"])           # overridden where the frame is calibrated
        g = dict(bboxes_3d=t(f["gt_boxes"]), labels_3d=t(f["gt_labels"]), neighbor=t(f["gt_neighbor"]),
                 occluded=t(f["gt_occluded"]), truncated=t(f["gt_truncated"]))
        if f.get("gt_height_given", True):
            g["bbox_height"] = t(f["gt_height"])
        if "lidar2img" in f:
            g["lidar2img"], g["img_shape"] = f["lidar2img"], f["img_shape"]
        for src, dst in (("gt_bbox", "bbox"), ("gt_alpha", "alpha"), ("dontcare", "dontcare")):
            if src in f:
                g[dst] = t(f[src])
        preds.append(p)
        gts.append(g)
    return preds, gts


def assert_equal_to_reference(counts, nthr, detail, want, fams, n_classes=3):
    """Every tp / fp / fn of every group of every family equals the reference's, and the thresholds' number."""
    G = n_classes * 6
    counts = counts.numpy()
    for (m, c, d, t), w in want.items():
        if m == "AOS":
            continue
        q = fams.index(m) * G + (c * 3 + d) * 2 + t
        assert nthr[q] == len(w["counts"]), (m, c, d, t, nthr[q], len(w["counts"]))
        assert [tuple(v) for v in counts[q, :nthr[q]].tolist()] == w["counts"], (m, c, d, t)
        assert not counts[q, nthr[q]:].any()
