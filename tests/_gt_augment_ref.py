"""Reference for the GT-database augmentation tests (TEST INFRASTRUCTURE ONLY).

Plain numpy float64, written from the specification in DESIGN.md "GT-database augmentation" with explicit
loops over frames, boxes, tries and candidates (vectorised over points only). Every function that takes a
decision can log the margin it decided on (`log`), so the case builders can keep all decisions away from
rounding noise: `inside` margins are signed distances to the nearest face (negative inside), collision
margins are the separating-axis `sep`.

Box = (x, y, z, dx, dy, dz, yaw), z the bottom face; a box exists iff label >= 0 and all extents > 0.
"""
from __future__ import annotations

import math

import numpy as np


def exists(box, label) -> bool:
    return bool(label >= 0 and box[3] > 0 and box[4] > 0 and box[5] > 0)


def inside_margin(points, box) -> np.ndarray:
    """Signed distance of each point [n, >=3] to the nearest face of `box` (negative inside; NaN for NaN points)."""
    p = np.asarray(points, np.float64)
    x, y, z, dx, dy, dz, yaw = (float(v) for v in box[:7])
    c, s = math.cos(yaw), math.sin(yaw)
    lx = (p[:, 0] - x) * c + (p[:, 1] - y) * s
    ly = -(p[:, 0] - x) * s + (p[:, 1] - y) * c
    lz = p[:, 2] - (z + dz / 2)
    return np.maximum(np.maximum(np.abs(lx) - dx / 2, np.abs(ly) - dy / 2), np.abs(lz) - dz / 2)


def inside(points, box) -> np.ndarray:
    """mmcv check_pt_in_box3d: strict in the box's plane, closed in z; a NaN point is inside nothing."""
    p = np.asarray(points, np.float64)
    x, y, z, dx, dy, dz, yaw = (float(v) for v in box[:7])
    c, s = math.cos(yaw), math.sin(yaw)
    lx = (p[:, 0] - x) * c + (p[:, 1] - y) * s
    ly = -(p[:, 0] - x) * s + (p[:, 1] - y) * c
    lz = p[:, 2] - (z + dz / 2)
    with np.errstate(invalid="ignore"):
        return (np.abs(lx) < dx / 2) & (np.abs(ly) < dy / 2) & (np.abs(lz) <= dz / 2)


def sep(a, b) -> float:
    """Separating-axis margin of the footprints (dx x dy rotated by yaw) of two boxes: the largest, over the
    four edge normals, of |projected centre distance| - sum of projected half extents."""
    best = -math.inf
    d = (float(b[0]) - float(a[0]), float(b[1]) - float(a[1]))
    rects = []
    for q in (a, b):
        yaw = float(q[6])
        ux, uy = (math.cos(yaw), math.sin(yaw)), (-math.sin(yaw), math.cos(yaw))
        rects.append((ux, uy, float(q[3]) / 2, float(q[4]) / 2))
    for r in rects:
        for axis in (r[0], r[1]):
            dist = abs(d[0] * axis[0] + d[1] * axis[1])
            ext = 0.0
            for ux, uy, hx, hy in rects:
                ext += hx * abs(ux[0] * axis[0] + ux[1] * axis[1]) + hy * abs(uy[0] * axis[0] + uy[1] * axis[1])
            best = max(best, dist - ext)
    return best


def collide(a, b, log=None) -> bool:
    v = sep(a, b)
    if log is not None:
        log.append(abs(v))
    return v < 0


# ------------------------------------------------------------------------------------------ points in boxes
def points_in_boxes_frame(points, boxes, labels):
    """One frame -> (first [n] (-1: none), contains [n, M] bool, counts [M])."""
    n, M = len(points), len(boxes)
    contains = np.zeros((n, M), bool)
    for m in range(M):
        if exists(boxes[m], labels[m]):
            contains[:, m] = inside(points, boxes[m])
    first = np.full(n, -1, np.int64)
    for m in range(M - 1, -1, -1):
        first[contains[:, m]] = m
    return first, contains, contains.sum(0)


def pack_mask(contains) -> np.ndarray:
    """[n, M] bool -> [n, ceil(M/32)] uint32, bit m % 32 of word m // 32."""
    n, M = contains.shape
    out = np.zeros((n, (M + 31) // 32), np.uint32)
    for m in range(M):
        out[:, m // 32] |= contains[:, m].astype(np.uint32) << np.uint32(m % 32)
    return out


def crop_objects(points, boxes, labels):
    """One frame's database objects: (box index, points centred on the box's (x, y, z), their row indices)."""
    out = []
    for m in range(len(boxes)):
        if not exists(boxes[m], labels[m]):
            continue
        idx = np.nonzero(inside(points, boxes[m]))[0]
        p = np.asarray(points, np.float64)[idx].copy()
        p[:, :3] -= np.asarray(boxes[m][:3], np.float64)
        out.append((m, p, idx))
    return out


# ------------------------------------------------------------------------------------------ ObjectSample
def sample_select(cand, draw, db_boxes, db_labels, gt_boxes, gt_labels, log=None):
    """One frame. cand / draw [S]; gt_boxes [M, 7] / gt_labels [M]. Returns (accept [S], boxes, labels)."""
    boxes = np.array(gt_boxes, np.float64)
    labels = np.array(gt_labels, np.int64)
    M, S = len(labels), len(cand)
    existing = [np.array(gt_boxes[m], np.float64) for m in range(M) if exists(gt_boxes[m], gt_labels[m])]
    accepted = []                      # candidate positions
    accept = np.full(S, -1, np.int64)
    for i in range(S):
        if cand[i] < 0:
            continue
        me = db_boxes[cand[i]]
        hit = False
        for e in existing:                                   # (a) the frame's own boxes
            hit = collide(me, e, log) or hit
        for k in accepted:                                   # (a) earlier draws, (b) earlier in this draw
            hit = collide(me, db_boxes[cand[k]], log) or hit
        for k in range(i + 1, S):                            # (c) every later candidate of this draw
            if cand[k] >= 0 and draw[k] == draw[i]:
                hit = collide(me, db_boxes[cand[k]], log) or hit
        if hit:
            continue
        free = [m for m in range(M) if labels[m] < 0]
        if not free:
            continue                                         # no slot left: rejected
        boxes[free[0]] = np.asarray(me, np.float64)
        labels[free[0]] = db_labels[cand[i]]
        accept[i] = free[0]
        accepted.append(i)
    return accept, boxes, labels


def sample_points(points, cand, accept, db_points, db_boxes):
    """One frame -> (pasted [k, F] float64, kept: row indices of the surviving scene points)."""
    pasted = []
    gone = np.zeros(len(points), bool)
    for i in range(len(cand)):
        if accept[i] < 0:
            continue
        box = np.asarray(db_boxes[cand[i]], np.float64)
        p = np.asarray(db_points[cand[i]], np.float64).copy()
        p[:, :3] += box[:3]
        pasted.append(p)
        gone |= inside(points, box)
    F = np.asarray(points).shape[1]
    pasted = np.concatenate(pasted, 0) if pasted else np.zeros((0, F))
    return pasted, np.nonzero(~gone)[0]


# ------------------------------------------------------------------------------------------ ObjectNoise
def noise_select(boxes, labels, loc, rot, log=None):
    """One frame. boxes [M, 7], loc [M, T, 3], rot [M, T] -> chosen [M]."""
    M, T = rot.shape
    cur = [np.array(boxes[m], np.float64) for m in range(M)]
    chosen = np.full(M, -1, np.int64)
    for i in range(M):
        if not exists(boxes[i], labels[i]):
            continue
        for j in range(T):
            tri = cur[i].copy()
            tri[0] += float(loc[i, j, 0])
            tri[1] += float(loc[i, j, 1])
            tri[6] += float(rot[i, j])
            hit = False
            for k in range(M):
                if k != i and exists(boxes[k], labels[k]):
                    hit = collide(tri, cur[k], log) or hit
            if not hit:
                chosen[i] = j
                cur[i] = tri
                break
    return chosen


def noise_apply(points, boxes, labels, loc, rot, chosen):
    """One frame -> (points float64, boxes float64, owner [n] (-1: none), moved [n] bool)."""
    p = np.array(points, np.float64)
    out = p.copy()
    owner, _, _ = points_in_boxes_frame(points, boxes, labels)
    moved = np.zeros(len(p), bool)
    nb = np.array(boxes, np.float64)
    for m in range(len(boxes)):
        j = chosen[m]
        if j < 0 or not exists(boxes[m], labels[m]):
            continue
        r, l = float(rot[m, j]), np.asarray(loc[m, j], np.float64)
        c, s = math.cos(r), math.sin(r)
        sel = owner == m
        dx, dy = p[sel, 0] - nb[m, 0], p[sel, 1] - nb[m, 1]
        out[sel, 0] = c * dx - s * dy + nb[m, 0] + l[0]
        out[sel, 1] = s * dx + c * dy + nb[m, 1] + l[1]
        out[sel, 2] = p[sel, 2] + l[2]
        moved |= sel
    for m in range(len(boxes)):
        j = chosen[m]
        if j >= 0:
            nb[m, :3] += np.asarray(loc[m, j], np.float64)
            nb[m, 6] += float(rot[m, j])
    return out, nb, owner, moved
