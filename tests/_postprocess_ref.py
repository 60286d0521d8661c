"""Float64 oracle of the detection post-processing (robustpointclouds_amd/postprocess.py and
csrc/postprocess.hip), as plain loops. It restates the specification, not the product code, and imports
nothing from the package.

Rotated BEV IoU: the corners of both boxes (after subtracting the centre of box a from both, a common
translation), box b clipped against the four edge half-planes of box a (Sutherland-Hodgman with cross
products), area by the shoelace formula. `bev_iou(a, b, dtype=np.float32)` runs the very same algorithm in
numpy float32 scalars: the independent fp32 reference the GPU test takes its tolerance from.
"""
from __future__ import annotations

import math

import numpy as np


# ----------------------------------------------------------------------------------- rotated IoU
def _corners(x, y, dx, dy, yaw, T, sin, cos):
    c, s = cos(yaw), sin(yaw)
    hx, hy = dx / T(2), dy / T(2)
    out = []
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):   # counter-clockwise
        lx, ly = T(sx) * hx, T(sy) * hy
        out.append((x + lx * c - ly * s, y + lx * s + ly * c))
    return out


def _clip_halfplane(poly, p, q, T):
    """The part of `poly` on the left of (or on) the directed line p -> q."""
    def side(v):
        return (q[0] - p[0]) * (v[1] - p[1]) - (q[1] - p[1]) * (v[0] - p[0])

    out = []
    n = len(poly)
    for k in range(n):
        cur, prv = poly[k], poly[k - 1]
        sc, sp = side(cur), side(prv)
        if (sc >= T(0)) != (sp >= T(0)):
            t = sp / (sp - sc)
            out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1])))
        if sc >= T(0):
            out.append(cur)
    return out


def _shoelace(poly, T):
    s = T(0)
    for k in range(len(poly)):
        s = s + (poly[k - 1][0] * poly[k][1] - poly[k][0] * poly[k - 1][1])
    return abs(s) / T(2)


def bev_iou(a, b, dtype=np.float64):
    """IoU of two (x, y, dx, dy, yaw) boxes; 0 if either has dx <= 0 or dy <= 0."""
    if dtype == np.float64:
        T, sin, cos = float, math.sin, math.cos
    else:
        T, sin, cos = dtype, np.sin, np.cos
    a = [T(v) for v in np.asarray(a, dtype=dtype)]
    b = [T(v) for v in np.asarray(b, dtype=dtype)]
    if not (a[2] > 0 and a[3] > 0 and b[2] > 0 and b[3] > 0):
        return T(0)
    pa = _corners(T(0), T(0), a[2], a[3], a[4], T, sin, cos)
    pb = _corners(b[0] - a[0], b[1] - a[1], b[2], b[3], b[4], T, sin, cos)
    poly = pb
    for k in range(4):
        poly = _clip_halfplane(poly, pa[k], pa[(k + 1) % 4], T)
        if not poly:
            break
    inter = _shoelace(poly, T) if len(poly) >= 3 else T(0)
    area_a, area_b = a[2] * a[3], b[2] * b[3]
    inter = min(inter, area_a, area_b)
    iou = inter / (area_a + area_b - inter)
    return min(max(iou, T(0)), T(1))


def iou_matrix(boxes):
    """Upper-triangular float64 IoU matrix of n boxes (pairs whose circumscribed circles are apart are 0
    without clipping: they cannot intersect)."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
    n = boxes.shape[0]
    m = np.zeros((n, n))
    rad = 0.5 * np.hypot(boxes[:, 2], boxes[:, 3])
    for i in range(n):
        d = np.hypot(boxes[i + 1:, 0] - boxes[i, 0], boxes[i + 1:, 1] - boxes[i, 1])
        for j in np.nonzero(d <= rad[i] + rad[i + 1:] + 1e-9)[0]:
            m[i, i + 1 + j] = bev_iou(boxes[i], boxes[i + 1 + j])
    return m


# ----------------------------------------------------------------------------------- greedy NMS
def greedy_nms(suppresses, n, max_keep=None):
    """suppresses(i, j) for i < j; boxes in score order. Returns the kept indices."""
    removed = [False] * n
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        if max_keep is not None and len(keep) >= max_keep:
            break
        keep.append(i)
        for j in range(i + 1, n):
            if not removed[j] and suppresses(i, j):
                removed[j] = True
    return keep


def nms_bev_sorted(boxes, thr, max_keep=None, iou=None):
    """boxes [n, 5] in descending score order; suppressed when IoU > thr (strict)."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 5)
    if iou is None:
        iou = iou_matrix(boxes)
    n = boxes.shape[0]
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        if max_keep is not None and len(keep) >= max_keep:
            break
        keep.append(i)
        removed[i + 1:] |= iou[i, i + 1:] > thr      # row i of the upper-triangular matrix
    return keep


def nms_bev(boxes, scores, thr, pre_max_size=None, post_max_size=None):
    """mmdet3d nms_bev: order by score, optional pre / post caps; indices into the input."""
    scores = np.asarray(scores, dtype=np.float64)
    order = np.argsort(-scores, kind="stable")
    if pre_max_size is not None:
        order = order[:pre_max_size]
    keep = nms_bev_sorted(np.asarray(boxes, dtype=np.float64)[order], thr)
    keep = order[keep]
    return keep[:post_max_size] if post_max_size is not None else keep


def circle_nms_sorted(xy, radius, max_keep=None):
    """mmdet3d circle_nms: squared distance <= (unsquared) radius suppresses; xy in score order."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)

    def sup(i, j):
        return (xy[i, 0] - xy[j, 0]) ** 2 + (xy[i, 1] - xy[j, 1]) ** 2 <= radius

    return greedy_nms(sup, xy.shape[0], max_keep)


def circle_nms(xy, scores, radius, post_max_size=None):
    order = np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")
    keep = order[circle_nms_sorted(np.asarray(xy, dtype=np.float64)[order], radius)]
    return keep[:post_max_size] if post_max_size is not None else keep


# ----------------------------------------------------------------------------------- Anchor3DHead
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def _limit_period(v, offset, period):
    return v - np.floor(v / period + offset) * period


def _delta_decode(anchors, deltas):
    xa, ya, za, wa, la, ha, ra = [anchors[:, k] for k in range(7)]
    xt, yt, zt, wt, lt, ht, rt = [deltas[:, k] for k in range(7)]
    za = za + ha / 2
    diag = np.sqrt(la ** 2 + wa ** 2)
    xg, yg, zg = xt * diag + xa, yt * diag + ya, zt * ha + za
    lg, wg, hg = np.exp(lt) * la, np.exp(wt) * wa, np.exp(ht) * ha
    return np.stack([xg, yg, zg - hg / 2, wg, lg, hg, rt + ra], axis=1)


def anchor_predict_single(cls, reg, dcl, anchors, num_classes, cfg, dir_offset, dir_limit_offset):
    """One frame of mmdet3d 1.x Anchor3DHead._predict_by_feat_single + box3d_multiclass_nms.
    cls [A*C, H, W], reg [A*7, H, W], dcl [A*2, H, W], anchors [H*W*A, 7].
    Returns (bboxes [n, 7], scores [n], labels [n], anchor_index [n])."""
    C = num_classes
    scores = _sigmoid(np.transpose(cls, (1, 2, 0)).reshape(-1, C))
    deltas = np.transpose(reg, (1, 2, 0)).reshape(-1, 7).astype(np.float64)
    dirl = np.argmax(np.transpose(dcl, (1, 2, 0)).reshape(-1, 2), axis=1)
    anchors = np.asarray(anchors, dtype=np.float64).reshape(-1, 7)
    index = np.arange(scores.shape[0])
    nms_pre = cfg.get("nms_pre", -1)
    if nms_pre > 0 and scores.shape[0] > nms_pre:
        top = np.argsort(-scores.max(axis=1), kind="stable")[:nms_pre]
        scores, deltas, dirl, anchors, index = scores[top], deltas[top], dirl[top], anchors[top], index[top]
    boxes = _delta_decode(anchors, deltas)
    bev = boxes[:, [0, 1, 3, 4, 6]]
    ob, osc, ol, od, oi = [], [], [], [], []
    for c in range(C):
        sel = np.nonzero(scores[:, c] > cfg["score_thr"])[0]
        if sel.size == 0:
            continue
        keep = sel[nms_bev(bev[sel], scores[sel, c], cfg["nms_thr"])]
        ob.append(boxes[keep]); osc.append(scores[keep, c]); ol.append(np.full(keep.size, c, dtype=np.int64))
        od.append(dirl[keep]); oi.append(index[keep])
    if not ob:
        return np.zeros((0, 7)), np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    ob, osc, ol, od, oi = (np.concatenate(v) for v in (ob, osc, ol, od, oi))
    if ob.shape[0] > cfg["max_num"]:
        top = np.argsort(-osc, kind="stable")[:cfg["max_num"]]
        ob, osc, ol, od, oi = ob[top], osc[top], ol[top], od[top], oi[top]
    ob = ob.copy()
    rot = _limit_period(ob[:, 6] - dir_offset, dir_limit_offset, np.pi)
    ob[:, 6] = rot + dir_offset + np.pi * od.astype(np.float64)
    return ob, osc, ol, oi


# ----------------------------------------------------------------------------------- CenterHead
def center_predict(hm, box, task_ncls, test_cfg, pc_range, norm_bbox=True):
    """mmdet3d 1.x CenterHead.predict_by_feat with nms_type='circle' over the packed head buffers
    hm [B, H, W, sum(ncls)], box [B, H, W, 10 * tasks]. Returns per frame (bboxes [n, 9], scores, labels)."""
    hm = np.asarray(hm, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    B, H, W, _ = hm.shape
    K = test_cfg["max_per_img"]
    osf, vs = test_cfg["out_size_factor"], test_cfg["voxel_size"]
    lim = test_cfg["post_center_limit_range"]
    thr = test_cfg.get("score_threshold")
    out = []
    for b in range(B):
        fb, fs, fl = [], [], []
        c0 = 0
        for t, n in enumerate(task_ncls):
            heat = _sigmoid(np.transpose(hm[b, :, :, c0:c0 + n], (2, 0, 1))).reshape(-1)
            top = np.argsort(-heat, kind="stable")[:K]
            bx, sc, lb = [], [], []
            for idx in top:
                cls, cell = divmod(int(idx), H * W)
                row, col = divmod(cell, W)
                v = box[b, row, col, 10 * t:10 * t + 10]
                x = (col + v[0]) * osf * vs[0] + pc_range[0]
                y = (row + v[1]) * osf * vs[1] + pc_range[1]
                z = v[2]
                dim = np.exp(v[3:6]) if norm_bbox else v[3:6]
                rot = math.atan2(v[6], v[7])
                ok = thr is None or heat[idx] > thr
                ok = ok and lim[0] <= x <= lim[3] and lim[1] <= y <= lim[4] and lim[2] <= z <= lim[5]
                if ok:
                    bx.append([x, y, z, dim[0], dim[1], dim[2], rot, v[8], v[9]])
                    sc.append(heat[idx]); lb.append(cls)
            bx = np.asarray(bx, dtype=np.float64).reshape(-1, 9)
            keep = circle_nms_sorted(bx[:, :2], test_cfg["min_radius"][t])[:test_cfg["post_max_size"]]
            fb.append(bx[keep]); fs.append(np.asarray(sc)[keep]); fl.append(np.asarray(lb, dtype=np.int64)[keep] + c0)
            c0 += n
        fb = np.concatenate(fb)
        fb[:, 2] = fb[:, 2] - fb[:, 5] * 0.5
        out.append((fb, np.concatenate(fs), np.concatenate(fl)))
    return out
