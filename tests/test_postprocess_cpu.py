"""Detection post-processing without a GPU: the float64 oracle (tests/_postprocess_ref.py) pinned to closed
forms, and the CPU paths of robustpointclouds_amd/postprocess.py and Anchor3DHead / CenterHead
`predict_by_feat` against that oracle."""
import math

import numpy as np
import pytest
import torch

from tests import _postprocess_cases as cs
from tests import _postprocess_ref as ref


# ----------------------------------------------------------------------------------- the oracle itself
def test_oracle_identical_and_disjoint():
    assert ref.bev_iou([3, -2, 4, 2, 0.7], [3, -2, 4, 2, 0.7]) == pytest.approx(1.0, abs=1e-12)
    assert ref.bev_iou([0, 0, 2, 2, 0.3], [10, 0, 2, 2, 1.1]) == 0.0
    assert ref.bev_iou([0, 0, 0, 2, 0], [0, 0, 2, 2, 0]) == 0.0
    assert ref.bev_iou([0, 0, 2, 2, 0], [0, 0, 2, -1, 0]) == 0.0


@pytest.mark.parametrize("ox,oy", [(0.5, 0.0), (1.0, 1.0), (1.5, -0.25), (3.0, 0.5)])
def test_oracle_axis_aligned_overlap(ox, oy):
    # a = [0, 4] x [0, 2] against the same box shifted by (ox, oy)
    ix, iy = max(0.0, 4 - abs(ox)), max(0.0, 2 - abs(oy))
    want = ix * iy / (16 - ix * iy)
    assert ref.bev_iou([2, 1, 4, 2, 0], [2 + ox, 1 + oy, 4, 2, 0]) == pytest.approx(want, abs=1e-12)
    # the same boxes described with length and width swapped and a quarter turn
    assert ref.bev_iou([2, 1, 2, 4, math.pi / 2], [2 + ox, 1 + oy, 4, 2, 0]) == pytest.approx(want, abs=1e-12)


def test_oracle_unit_square_rotated_45():
    inter = 2 * (math.sqrt(2) - 1)            # the regular octagon
    want = (2 * math.sqrt(2) - 2) / (4 - 2 * math.sqrt(2))
    assert want == pytest.approx(inter / (2 - inter), abs=1e-15)
    assert ref.bev_iou([0, 0, 1, 1, 0], [0, 0, 1, 1, math.pi / 4]) == pytest.approx(want, abs=1e-12)


def test_oracle_invariances():
    a, b = cs.random_pairs(64, seed=5)
    a, b = a.astype(np.float64), b.astype(np.float64)
    th, tx, ty = 0.83, 12.5, -7.25
    c, s = math.cos(th), math.sin(th)

    def moved(v):
        return [c * v[0] - s * v[1] + tx, s * v[0] + c * v[1] + ty, v[2], v[3], v[4] + th]

    def mirrored(v):
        return [v[0], -v[1], v[2], v[3], -v[4]]

    some = 0
    for x, y in zip(a, b):
        i = ref.bev_iou(x, y)
        some += i > 0
        assert ref.bev_iou(moved(x), moved(y)) == pytest.approx(i, abs=1e-9)
        assert ref.bev_iou(mirrored(x), mirrored(y)) == pytest.approx(i, abs=1e-9)
        assert ref.bev_iou(y, x) == pytest.approx(i, abs=1e-9)
    assert some > 16


def test_oracle_degenerate_table():
    a, b, want = cs.degenerate_pairs()
    for x, y, w in zip(a, b, want):
        i = ref.bev_iou(x, y)
        assert 0.0 <= i <= 1.0
        if w is not None:
            assert i == pytest.approx(w, abs=1e-6)   # the table is rounded to fp32


# ----------------------------------------------------------------------------------- the package's CPU path
def test_cpu_iou_pairs_match_oracle():
    from robustpointclouds_amd import postprocess as pp
    a, b = cs.random_pairs(256, seed=2)
    da, db, _ = cs.degenerate_pairs()
    a, b = np.concatenate([a, da]), np.concatenate([b, db])
    got = pp.bev_iou_pairs(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    want = np.array([ref.bev_iou(x, y) for x, y in zip(a, b)])
    assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    assert np.abs(got - want).max() < 1e-6


@pytest.mark.parametrize("thr", [0.01, 0.2, 0.5])
def test_cpu_nms_bev_matches_oracle(thr):
    from robustpointclouds_amd import postprocess as pp
    boxes, counts, ious, _ = cs.nms_groups(thr, seed=0, counts=[0, 1, 2, 40])
    keep, nkeep = pp.nms_bev_batched(torch.from_numpy(boxes), torch.tensor(counts), thr)
    for g, n in enumerate(counts):
        want = ref.nms_bev_sorted(boxes[g, :n], thr, iou=ious[g])
        assert int(nkeep[g]) == len(want)
        assert keep[g, :len(want)].tolist() == want
        assert (keep[g, len(want):] == -1).all()
    # the single-set form: unsorted input, caps
    r = np.random.RandomState(3)
    n = counts[-1]
    scores = r.permutation(n).astype(np.float64)
    b = boxes[-1, :n]
    got = pp.nms_bev(torch.from_numpy(b), torch.from_numpy(scores), thr, pre_max_size=30, post_max_size=7)
    want = ref.nms_bev(b, scores, thr, pre_max_size=30, post_max_size=7)
    assert got.dtype == torch.int64 and got.tolist() == want.tolist()


def test_cpu_circle_nms_matches_oracle():
    from robustpointclouds_amd import postprocess as pp
    counts = [0, 1, 2, 63, 64, 65]
    xy, counts = cs.circle_groups(counts)
    rad = torch.tensor(cs.NUS_MIN_RADIUS, dtype=torch.float32)
    keep, nkeep = pp.nms_circle_batched(torch.from_numpy(xy), torch.tensor(counts), rad, max_keep=30)
    for g, n in enumerate(counts):
        want = ref.circle_nms_sorted(xy[g, :n], cs.NUS_MIN_RADIUS[g], max_keep=30)
        assert int(nkeep[g]) == len(want) and keep[g, :len(want)].tolist() == want
    n = counts[3]
    scores = np.random.RandomState(4).permutation(n).astype(np.float64)
    got = pp.circle_nms(torch.from_numpy(xy[3, :n]), torch.from_numpy(scores), 1.0, post_max_size=9)
    assert got.tolist() == ref.circle_nms(xy[3, :n], scores, 1.0, post_max_size=9).tolist()


@pytest.mark.parametrize("max_num", [5, 50])
def test_cpu_anchor_predict_by_feat(max_num):
    """3-class head, H = W = 4, 6 anchors per cell, nms_pre = 20: candidates with two labels, the max_num cap
    (5: the score-ordered branch; 50: the class-major branch) and the direction correction; one frame without
    any detection."""
    head = cs.kitti_head()
    cfg = dict(head.test_cfg, nms_pre=20, max_num=max_num)
    cls, reg, dcl = cs.head_maps(2, 4, 4, seed=1, bias=(-3.0, -12.0))
    want = cs.anchor_oracle(head, cls, reg, dcl, cfg)
    assert cs.distinct(want[0][1])
    uncapped = cs.anchor_oracle(head, cls, reg, dcl, dict(cfg, max_num=10 ** 6))[0]
    assert len(uncapped[3]) > len(set(uncapped[3].tolist()))          # an anchor kept under two classes
    assert len(uncapped[2]) > 5 and len(want[0][2]) == min(max_num, len(uncapped[2])) and len(want[1][2]) == 0
    assert len(set(uncapped[2].tolist())) == 3
    got = head.predict_by_feat([cls], [reg], [dcl], cfg)
    cs.check_detections(got, want)
    # the direction bin moved some yaw by pi: without it the oracle's own boxes differ
    assert set(np.unique(np.argmax(dcl[0].permute(1, 2, 0).reshape(-1, 2).numpy(), 1))) == {0, 1}


def test_cpu_anchor_predict_options():
    head = cs.kitti_head()
    cls, reg, dcl = cs.head_maps(1, 4, 4, seed=1)
    with pytest.raises(NotImplementedError, match="use_rotate_nms"):
        head.predict_by_feat([cls], [reg], [dcl], dict(head.test_cfg, use_rotate_nms=False))
    # nms_pre off: every anchor is a candidate
    cfg = dict(head.test_cfg, nms_pre=-1, max_num=500, score_thr=0.3)
    cs.check_detections(head.predict_by_feat(cls, reg, dcl, cfg), cs.anchor_oracle(head, cls, reg, dcl, cfg))


def test_cpu_center_predict_by_feat():
    head = cs.center_head()
    hm, box = cs.center_buffers()
    B, H, W, _ = hm.shape
    preds = ([dict(_packed=(hm.view(B * H * W, -1), box.view(B * H * W, -1), B, H, W))],)
    got = head.predict_by_feat(preds)
    want = ref.center_predict(hm.numpy(), box.numpy(), head.num_classes, head.test_cfg,
                              head.train_cfg["point_cloud_range"])
    cs.check_detections(got, want)
    for w in want:
        assert cs.distinct(w[1]) and 0 < len(w[2]) <= 10
        assert set(w[2].tolist()) - {0} and (w[2] <= 2).all()            # labels of the second task are offset
    with pytest.raises(NotImplementedError, match="rotate"):
        head.predict_by_feat(preds, dict(head.test_cfg, nms_type="rotate"))
