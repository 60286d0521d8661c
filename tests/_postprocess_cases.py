"""Seeded inputs shared by tests/test_postprocess_cpu.py and tests/test_gpu_postprocess.py."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from tests import _postprocess_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
NUS_MIN_RADIUS = [4, 12, 10, 1, 0.85, 0.175]
NMS_COUNTS = [0, 1, 2, 63, 64, 65, 130, 1000]


def kitti_cfg():
    with open(os.path.join(HERE, "golden", "config_kitti3class.json")) as f:
        return json.load(f)["model"]


def kitti_head(test_cfg=None):
    """The KITTI 3-class Anchor3DHead of the golden config (6 anchors per cell), parameters unused."""
    from robustpointclouds_amd.anchor_head import Anchor3DHead
    m = kitti_cfg()
    hc = dict(m["bbox_head"])
    hc.pop("type")
    return Anchor3DHead(**hc, train_cfg=m.get("train_cfg"), test_cfg=test_cfg or m["test_cfg"])


def head_maps(B, H, W, seed, bias=(-3.0,), A=6, C=3):
    """Seeded head maps: class logits N(bias[b], 2) (about a third above score_thr = 0.1 at bias -3, none at
    -12), box deltas N(0, 0.3), dir logits N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    bias = torch.tensor([bias[b % len(bias)] for b in range(B)], dtype=torch.float32).view(B, 1, 1, 1)
    cls = torch.randn((B, A * C, H, W), generator=g) * 2.0 + bias
    reg = torch.randn((B, A * 7, H, W), generator=g) * 0.3
    dcl = torch.randn((B, A * 2, H, W), generator=g)
    return cls, reg, dcl


def anchor_oracle(head, cls, reg, dcl, cfg):
    """tests/_postprocess_ref.anchor_predict_single per frame, on the head's own anchors."""
    B, _, H, W = cls.shape
    anchors = head.anchors((H, W), "cpu").reshape(-1, 7).double().numpy()
    return [ref.anchor_predict_single(cls[b].double().cpu().numpy(), reg[b].double().cpu().numpy(),
                                      dcl[b].double().cpu().numpy(), anchors, head.num_classes, cfg,
                                      float(head.dir_offset), float(head.dir_limit_offset)) for b in range(B)]


def check_detections(got, want, atol=1e-5):
    """got: predict_by_feat's per-frame dicts; want: the oracle's (boxes, scores, labels, ...) tuples. Labels,
    order and counts exact; boxes and scores to `atol` absolute."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g["labels_3d"].dtype == torch.int64
        assert g["labels_3d"].cpu().tolist() == w[2].tolist()
        assert tuple(g["bboxes_3d"].shape) == w[0].shape and tuple(g["scores_3d"].shape) == w[1].shape
        if w[0].shape[0]:
            assert np.abs(g["bboxes_3d"].double().cpu().numpy() - w[0]).max() <= atol
            assert np.abs(g["scores_3d"].double().cpu().numpy() - w[1]).max() <= atol


def distinct(scores) -> bool:
    s = np.sort(np.asarray(scores, dtype=np.float64).reshape(-1))
    return bool((np.diff(s) > 0).all())


def random_pairs(n, seed):
    """n pairs of BEV boxes: centres in +-80 m, sizes 0.3-12 m, any yaw; about half of the pairs overlap (the
    second centre lies within the first box's reach), the others are independent."""
    r = np.random.RandomState(seed)
    a = np.stack([r.uniform(-80, 80, n), r.uniform(-80, 80, n), r.uniform(0.3, 12, n), r.uniform(0.3, 12, n),
                  r.uniform(-np.pi, np.pi, n)], 1)
    b = np.stack([r.uniform(-80, 80, n), r.uniform(-80, 80, n), r.uniform(0.3, 12, n), r.uniform(0.3, 12, n),
                  r.uniform(-2 * np.pi, 2 * np.pi, n)], 1)
    near = r.rand(n) < 0.55
    off = r.uniform(-0.5, 0.5, (n, 2)) * np.maximum(a[:, 2:4], b[:, 2:4])
    b[near, :2] = a[near, :2] + off[near]
    return a.astype(np.float32), b.astype(np.float32)


def degenerate_pairs():
    """(a, b, expected IoU or None)."""
    h = np.pi / 2
    rows = [
        ([10, 20, 4, 2, 0.3], [10, 20, 4, 2, 0.3], 1.0),                    # identical
        ([-70, 65, 3.9, 1.6, 1.57], [-70, 65, 3.9, 1.6, 1.57], 1.0),
        ([0, 0, 4, 4, 0], [0.5, -0.5, 1, 1, 0], 1.0 / 16.0),                # containment
        ([0, 0, 6, 6, 0.7], [0.2, 0.1, 1, 2, 0.7], 2.0 / 36.0),
        ([0, 0, 2, 2, 0], [2, 0, 2, 2, 0], 0.0),                            # shared edge
        ([0, 0, 2, 2, 0], [2, 2, 2, 2, 0], 0.0),                            # shared corner
        ([5, 5, 4, 2, 0.25], [5.5, 5, 4, 2, 0.25], None),                   # yaw difference exactly 0
        ([5, 5, 4, 2, 0], [5, 5, 2, 4, h], None),                           # pi / 2
        ([5, 5, 4, 2, 0], [5, 5, 4, 2, np.pi], None),                       # pi
        ([0, 0, 0, 2, 0], [0, 0, 2, 2, 0], 0.0),                            # dx = 0
        ([0, 0, 2, 2, 0], [0, 0, 2, -1, 0], 0.0),                           # negative dy
        ([30, -40, 1e-3, 5, 0.4], [30, -40, 5, 1e-3, 0.4], None),           # slivers
        ([30, -40, 1e-3, 5, 0.4], [30.0002, -40, 1e-3, 5, 0.4], None),
        ([30, -40, 5, 1e-3, 1.0], [30, -40, 6, 4, -0.5], None),
    ]
    a = np.asarray([r[0] for r in rows], dtype=np.float32)
    b = np.asarray([r[1] for r in rows], dtype=np.float32)
    return a, b, [r[2] for r in rows]


def nms_groups(thr, seed=0, counts=NMS_COUNTS, margin=1e-4):
    """Score-ordered BEV boxes for each group count, about 6 overlapping neighbours per box, around
    (60, -30) m. The lower-scored box of every pair whose float64 IoU is within `margin` of `thr` is dropped
    (the kernel's fp32 IoU error with local-frame clipping is ~1e-5 there), from 5 % spare boxes, so that the
    counts stay. -> (boxes [G, max_n, 5] fp32 zero-padded, counts, per-group float64 IoU matrices, largest
    fraction of a group dropped)."""
    r = np.random.RandomState(1000 + seed)
    max_n = max(counts)
    out = np.zeros((len(counts), max_n, 5), dtype=np.float32)
    ious, worst = [], 0.0
    for g, n in enumerate(counts):
        m = n + (n + 19) // 20 + (1 if n else 0)
        ext = max(np.sqrt(3.0 * max(n, 1)), 3.0)
        b = np.stack([60 + r.uniform(0, ext, m), -30 + r.uniform(0, ext, m), r.uniform(1.5, 4.5, m),
                      r.uniform(0.8, 2.5, m), r.uniform(-np.pi, np.pi, m)], 1).astype(np.float32)
        iou = ref.iou_matrix(b)
        amb = np.nonzero(np.abs(iou - thr) < margin)
        drop = np.zeros(m, dtype=bool)
        drop[amb[1]] = True                 # the matrix is upper-triangular: the column is the lower score
        worst = max(worst, drop.sum() / max(m, 1))
        sel = np.nonzero(~drop)[0][:n]
        assert sel.size == n
        out[g, :n] = b[sel]
        ious.append(iou[np.ix_(sel, sel)])
    return out, list(counts), ious, worst


CIRCLE_COUNTS = ([0, 1, 2, 63, 64, 65], [65, 130, 1000, 64, 63, 2])


def circle_groups(counts, radii=NUS_MIN_RADIUS, seed=0):
    """Centres in score order on an integer grid (a 0.5 m grid under the radii below 1), so that squared
    distances are exact in fp32 and `<=` is decidable; the grid is dense enough that pairs at squared distance
    exactly equal to the radii 4, 10 and 1 occur in every group of 63 boxes or more."""
    r = np.random.RandomState(2000 + seed)
    max_n = max(counts)
    xy = np.zeros((len(counts), max_n, 2), dtype=np.float32)
    for g, n in enumerate(counts):
        step = 0.5 if radii[g] < 1 else 1.0
        ext = max(int(np.sqrt(0.7 * max(n, 1) * max(radii[g] / step ** 2, 1))), 3)
        xy[g, :n] = r.randint(-ext, ext + 1, (n, 2)) * step + np.array([40, -25])
    return xy, list(counts)


def center_buffers(B=2, H=16, W=16, tasks=(1, 2), seed=0):
    """Packed CenterHead buffers hm [B, H, W, sum(tasks)], box [B, H, W, 10 * len(tasks)]: heatmap logits
    N(-4.2, 1.5) (a share of the first task's top 40 below score_threshold 0.1), reg in [0, 1), heights around -1 with some beyond
    +-10 (outside post_center_limit_range in z), log-dims N(0.5, 0.3), any rotation, velocities N(0, 1)."""
    g = torch.Generator().manual_seed(3000 + seed)
    T = len(tasks)
    hm = torch.randn((B, H, W, sum(tasks)), generator=g) * 1.5 - 4.2
    box = torch.zeros((B, H, W, T, 10))
    box[..., 0:2] = torch.rand((B, H, W, T, 2), generator=g)
    hei = torch.randn((B, H, W, T), generator=g) - 1.0
    far = torch.rand((B, H, W, T), generator=g) < 0.1
    box[..., 2] = torch.where(far, hei * 30.0, hei)
    box[..., 3:6] = torch.randn((B, H, W, T, 3), generator=g) * 0.3 + 0.5
    box[..., 6:8] = torch.randn((B, H, W, T, 2), generator=g)
    box[..., 8:10] = torch.randn((B, H, W, T, 2), generator=g)
    return hm.contiguous(), box.reshape(B, H, W, T * 10).contiguous()


CENTER_TEST_CFG = dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_per_img=40,
                       max_pool_nms=False, min_radius=[4, 0.85], score_threshold=0.1, out_size_factor=8,
                       voxel_size=[0.1, 0.1], nms_type="circle", pre_max_size=1000, post_max_size=5, nms_thr=0.2)


def center_head(tasks=(1, 2)):
    """A CenterHead with the given classes per task; the grid's first columns lie west of
    post_center_limit_range."""
    from robustpointclouds_amd.center_head import NUS_TRAIN_CFG, CenterHead
    names = [["c%d_%d" % (t, k) for k in range(n)] for t, n in enumerate(tasks)]
    tc = dict(NUS_TRAIN_CFG, point_cloud_range=[-66.0, -58.0, -5.0, 36.4, 44.4, 3.0])
    return CenterHead(in_channels=64, tasks=[dict(num_class=len(n), class_names=n) for n in names], train_cfg=tc,
                      test_cfg=dict(CENTER_TEST_CFG))
