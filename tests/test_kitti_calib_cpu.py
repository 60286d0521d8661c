"""The calibration side of the KITTI evaluator on the CPU path (robustpointclouds_amd/kitti_eval.py: read_calib,
lidar2img, the projection, the detection filter, the 2D `bbox` metric with DontCare regions, AOS) against hand
values and the float64 restatement tests/_kitti_calib_ref.py; and every margin of the GPU test's cases."""
import math

import numpy as np
import pytest
import torch

from robustpointclouds_amd import kitti_eval as ke
from tests import _kitti_calib_cases as cc
from tests import _kitti_calib_ref as cref
from tests import _kitti_eval_cases as cs

FOUR = ("BEV", "3D", "2D", "AOS")
HW = (400, 1000)


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype)))


# ----------------------------------------------------------------------------------- calibration files
def test_read_calib_and_lidar2img(tmp_path):
    P2, R0, Tr = cc.calibration(3)
    lines = ["P0: " + " ".join(["1.0"] * 12), "P2: " + " ".join(repr(float(v)) for v in P2.reshape(-1)),
             "R0_rect: " + " ".join(repr(float(v)) for v in R0.reshape(-1)),
             "Tr_velo_to_cam: " + " ".join(repr(float(v)) for v in Tr.reshape(-1)), "Tr_imu_to_velo: " + "0 " * 12, ""]
    path = tmp_path / "000007.txt"
    path.write_text("\n".join(lines))
    got = ke.read_calib(str(path))
    assert set(got) == {"P2", "R0_rect", "Tr_velo_to_cam"}
    for key, want in (("P2", P2), ("R0_rect", R0), ("Tr_velo_to_cam", Tr)):
        assert got[key].dtype == np.float64 and got[key].shape == want.shape and np.array_equal(got[key], want)
    bad = tmp_path / "bad.txt"
    bad.write_text("\n".join(l for l in lines if not l.startswith("R0_rect")))
    with pytest.raises(ValueError):
        ke.read_calib(str(bad))
    short = tmp_path / "short.txt"
    short.write_text("\n".join(l if not l.startswith("P2") else "P2: 1 2 3" for l in lines))
    with pytest.raises(ValueError):
        ke.read_calib(str(short))
    # the hand product: P2 (3 x 4) . [R0 0; 0 1] . [Tr; 0 0 0 1]
    m = ke.lidar2img(P2, R0, Tr)
    want = np.zeros((3, 4))
    R4 = [[R0[i][j] if i < 3 and j < 3 else float(i == j) for j in range(4)] for i in range(4)]
    T4 = [list(Tr[i]) for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]]
    for i in range(3):
        for j in range(4):
            want[i, j] = sum(P2[i][a] * R4[a][b] * T4[b][j] for a in range(4) for b in range(4))
    assert m.dtype == np.float32 and m.shape == (3, 4)
    assert np.abs(m.astype(np.float64) - want).max() <= 2.0 ** -24 * np.abs(want).max()
    assert np.array_equal(m, cref.lidar2img(P2, R0, Tr))
    assert np.array_equal(ke.lidar2img(P2, np.eye(3), np.hstack([np.eye(3), np.zeros((3, 1))])), P2.astype(np.float32))


# ----------------------------------------------------------------------------------- hand projections
def _project(boxes, hw=HW):
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 7)
    out = ke.project_boxes(_t(boxes), [0, len(boxes)], _t(cc.identity_like()).reshape(1, 12), _t([hw]))
    return {k: v.numpy() for k, v in out.items()}


def test_hand_projections():
    """u = 500 + 100 y / x, v = 200 + 100 z / x (tests/_kitti_calib_cases.identity_like), image 400 x 1000."""
    boxes = [
        [10, 0, -1, 2, 4, 2, 0],          # straight ahead: near face x = 9, far face x = 11
        [10, 80, -1, 2, 4, 2, 0],         # wholly right of the image (u > 1000): invalid
        [10, -80, -1, 2, 4, 2, 0],        # wholly left of the image (u < 0): invalid
        [2, 9.5, -2.9, 2, 4, 2.8, 0],     # clipped at two edges (right and top)
        [10, 0, -3.5, 2, 4, 2, 0],        # below z = -3: invalid
        [math.nan, 0, -1, 2, 4, 2, 0],    # NaN: invalid
        [80, 0, -1, 2, 4, 2, 0],          # beyond x = 70.4: invalid
        [1, 0, -1, 4, 2, 2, 0],           # across the camera plane: corners at x = -1 divide by a negative W
    ]
    p = _project(boxes)
    assert p["valid"].tolist() == [True, False, False, True, False, False, False, True]
    # box 0: y in [-2, 2], z in [-1, 1]; the extremes come from the near face x = 9
    want = [500 - 200 / 9, 200 - 100 / 9, 500 + 200 / 9, 200 + 100 / 9]
    assert np.abs(p["raw"][0] - want).max() < 1e-4 and np.abs(p["clip"][0] - want).max() < 1e-4
    assert abs(p["height"][0] - 200 / 9) < 1e-4
    assert p["raw"][1][0] > 1000 and p["raw"][2][2] < 0
    # box 3: x in [1, 3], y in [7.5, 11.5], z in [-2.9, -0.1]: u in [750, 1650], v in [-90, 196.67]
    assert np.abs(p["raw"][3] - [500 + 750 / 3, 200 - 290 / 1, 500 + 1150 / 1, 200 - 10 / 3]).max() < 1e-3
    assert np.abs(p["clip"][3] - [750, 0, 1000, 200 - 10 / 3]).max() < 1e-3 and abs(p["height"][3] - (200 - 10 / 3)) < 1e-3
    assert np.isnan(p["raw"][5]).all() and (p["clip"][5] == 0).all() and p["height"][5] == 0
    # box 7: x in [-1, 3], y in [-1, 1], z in [-1, 1]: u = 500 + 100 y / x spans [400, 600] (x = -1 and x = 3 give
    # 500 -+ 100 and 500 -+ 33.3); no depth test, so the corners behind the camera count
    assert np.abs(p["raw"][7] - [400, 100, 600, 300]).max() < 1e-3
    # the float64 reference agrees on every finite row
    for k, b in enumerate(boxes):
        r = cref.project(np.float32(b), cc.identity_like(), HW)
        assert r["valid"] == bool(p["valid"][k])
        if np.isfinite(r["raw"]).all():
            assert np.abs(p["raw"][k] - r["raw"]).max() < 1e-3 and abs(p["height"][k] - r["height"]) < 1e-3
    # rows past the last offset belong to no frame
    out = ke.project_boxes(_t(boxes), [0, 2], _t(cc.identity_like()).reshape(1, 12), _t([HW]))
    assert out["valid"].tolist() == [True, False] + [False] * 6 and (out["raw"][2:] == 0).all()


def test_hand_alpha():
    """alpha = atan2(y, x) - yaw - pi / 2: on the x axis facing +x it is -pi / 2; at 45 degrees facing +x, -pi / 4;
    at 45 degrees facing along the ray, -pi / 2 again."""
    p = _project([[10, 0, -1, 2, 2, 2, 0], [10, 10, -1, 2, 2, 2, 0], [10, 10, -1, 2, 2, 2, math.pi / 4]])
    assert p["alpha"].dtype == np.float64
    yaw45 = float(np.float32(math.pi / 4))
    assert np.abs(p["alpha"] - [-math.pi / 2, math.pi / 4 - math.pi / 2, math.pi / 4 - yaw45 - math.pi / 2]).max() < 1e-12


def test_iou_2d_hand_values():
    d, g, wants = cc.degenerate_2d()
    off = list(range(len(d) + 1))
    ov, ov_off = ke.box_overlaps_2d(_t(d), off, _t(g), off)
    assert ov_off == off
    for k, w in enumerate(wants):
        ref = cref.iou_2d(g[k], d[k])
        if w is not None:
            assert float(ov[k]) == w and ref == w, (k, float(ov[k]), ref)    # 1, 0, 1/2, 1/4: exact
        else:
            assert abs(float(ov[k]) - ref) < 1e-6
    a = _t([[0, 0, 10, 10], [5, 5, 15, 15]])
    ov, _ = ke.box_overlaps_2d(a, [0, 2], a, [0, 2])
    assert np.allclose(ov.view(2, 2).numpy(), [[1, 25 / 175], [25 / 175, 1]], atol=1e-7)


def test_dontcare_bits_hand_values():
    """A detection half inside a DontCare box: ratio 0.5, stuff for a minimum overlap below 0.5 only."""
    det = _t([[0, 0, 100, 100], [200, 0, 300, 100], [0, 0, 0, 50]])
    dc = _t([[50, 0, 400, 100]])
    bits = ke.box_overlaps_2d(det, [0, 3], dc, [0, 1], mode=1, min_overlaps=[0.7, 0.5, 0.25])
    assert bits.dtype == torch.uint8 and bits.tolist() == [[0, 1, 0], [0, 1, 0], [1, 1, 0]]
    with pytest.raises(ValueError):
        ke.box_overlaps_2d(det, [0, 3], torch.zeros(65, 4), [0, 65], mode=1, min_overlaps=[0.5])


# ----------------------------------------------------------------------------------- the matcher's new branches
def _calib_frame(det_boxes, scores, gt_boxes, **kw):
    fr = cs.frame(det_boxes, scores, [0] * len(scores), gt_boxes, [0] * len(gt_boxes))
    fr["lidar2img"], fr["img_shape"] = cc.identity_like(), HW
    fr["gt_height_given"] = False
    fr.update(kw)
    return fr


def _compute(frames, metrics=FOUR, **kw):
    m = ke.KittiAP(["Car"], metrics=metrics, **kw)
    m.update(*cc.to_update(frames, with_height=False))
    detail = {}
    counts, nthr = m._counts(detail=detail)
    return m.compute(), counts, nthr, detail


def test_stuff_detection_is_no_false_positive_but_can_take_a_ground_truth():
    """Detection 0 sits on ground truth 0 (u in [467, 533]), detection 1, of the higher score, on nothing (u in
    [655, 756]), inside a DontCare box:
    without the region tp = 1, fp = 1; with it fp = 0. A DontCare box over detection 0 changes nothing: it still
    takes its ground truth and is a true positive."""
    big = lambda y: [10, y, -2.5, 2, 6, 4, 0]                   # about 60 px wide and 44 px high (near face x = 9)
    frames = lambda dc: [_calib_frame([big(0), big(20)], [0.8, 0.9], [big(0)], dontcare=np.asarray(dc, np.float32))]
    free, *_ = _compute(frames(np.zeros((0, 4))))
    _, c_free, nthr, _ = _compute(frames(np.zeros((0, 4))))
    with_dc, c_dc, _, d_dc = _compute(frames([[600, 0, 1000, 400]]))
    _, c_on, _, _ = _compute(frames([[300, 0, 580, 400]]))
    G, k2d = 6, 2
    row = k2d * G + 2                    # family 2D, class 0, moderate, strict
    assert nthr[row] == 1
    assert c_free[row, 0].tolist() == [1, 1, 0]
    assert c_dc[row, 0].tolist() == [1, 0, 0] and d_dc["stuff"].tolist() == [[0, 1]]
    assert c_on[row, 0].tolist() == [1, 1, 0]
    assert c_dc[2, 0].tolist() == [1, 1, 0]            # BEV does not look at DontCare regions
    assert abs(free["KITTI/Car_2D_AP11_moderate_strict"] - 50.0 / 11.0) < 1e-9       # precision 1 / 2
    assert abs(with_dc["KITTI/Car_2D_AP11_moderate_strict"] - 100.0 / 11.0) < 1e-9
    assert abs(with_dc["KITTI/Car_BEV_AP11_moderate_strict"] - 50.0 / 11.0) < 1e-9


@pytest.mark.parametrize("delta, factor", [(0.0, 1.0), (math.pi / 2, 0.5), (math.pi, 0.0)])
def test_aos_against_ap_for_known_angle_differences(delta, factor):
    """hand_41's geometry seen by the camera: 41 matched pairs, precision 1 everywhere. With every detection
    turned by delta against its ground truth's annotated angle, AOS = AP (1 + cos delta) / 2."""
    gts = [[5.0, float(k - 20), -2.95, 0.8, 0.8, 2.9, 0.3] for k in range(41)]     # 16 px wide, 20 px apart, 60 px high
    fr = _calib_frame(gts, [0.95 - 0.02 * k for k in range(41)], gts)
    det_alpha = cref.prepare([fr])[0]["det_alpha"]
    fr["gt_alpha"] = det_alpha + delta
    got, counts, nthr, detail = _compute([fr])
    for d in ("easy", "moderate", "hard"):
        ap = got[f"KITTI/Car_2D_AP40_{d}_strict"]
        assert abs(got[f"KITTI/Car_AOS_AP40_{d}_strict"] - factor * ap) < 1e-8, d
        assert abs(got[f"KITTI/Car_AOS_AP11_{d}_loose"] - factor * got[f"KITTI/Car_2D_AP11_{d}_loose"]) < 1e-8
    assert got["KITTI/Car_2D_AP40_hard_strict"] == 100.0
    want = cref.result_dict(cref.evaluate(cref.prepare([fr]), ["Car"]), ["Car"])
    assert set(got) == set(want) and max(abs(got[k] - want[k]) for k in want) < 1e-9


def test_default_metric_returns_the_old_keys_and_values():
    """No calibration, default arguments: the key set and every value of the evaluator before the calibration."""
    frames = list(cs.branch_frames().values()) + cs.random_frames(6, seed=1, cap_frame=False)
    m = ke.KittiAP(cs.CLASSES)
    m.update(*cs.to_update(frames))
    got = m.compute()
    keys = {f"KITTI/{c}_{x}_AP{r}_{d}_{t}" for c in cs.CLASSES for x in ("BEV", "3D") for r in (11, 40)
            for d in ("easy", "moderate", "hard") for t in ("strict", "loose")}
    keys |= {f"KITTI/Overall_{x}_AP{r}_{d}" for x in ("BEV", "3D") for r in (11, 40) for d in ("easy", "moderate", "hard")}
    assert set(got) == keys and list(got)[0] == "KITTI/Car_BEV_AP11_easy_strict"
    from tests import _kitti_eval_ref as kref
    want = kref.result_dict(kref.evaluate(frames, cs.CLASSES), cs.CLASSES)
    assert max(abs(got[k] - want[k]) for k in want) < 1e-9
    assert ke.KittiAP(cs.CLASSES, metrics=("AOS",)).metrics == ("AOS",) and len(ke.KittiAP(cs.CLASSES, metrics=FOUR).compute()) == 2 * len(keys)
    with pytest.raises(ValueError):
        ke.KittiAP(cs.CLASSES, metrics=("bbox",))
    with pytest.raises(ValueError):      # 2D without a calibration or 2D boxes on both sides
        ke.KittiAP(cs.CLASSES, metrics=("2D",)).update(*cs.to_update(frames[:1]))
    # 2D boxes on both sides stand in for the calibration
    p, g = cs.to_update([cs.hand_single()[0]])
    p[0]["bbox"], g[0]["bbox"] = _t([[10, 10, 60, 90]]), _t([[10, 10, 60, 90]])
    m = ke.KittiAP(["Car"], metrics=("2D", "AOS"))
    m.update(p, g)
    out = m.compute()
    assert abs(out["KITTI/Car_2D_AP11_hard_strict"] - 100.0 / 11.0) < 1e-9 and len(out) == 2 * 18


def test_calibrated_heights_make_the_difficulties_differ():
    """Ground truth 0 is 60 px high, ground truth 1 (further away) 30 px: easy (> 40 px) counts one valid ground
    truth, moderate (> 25 px) two, and the single detection sits on the far one."""
    near, far = [10, -3, -2.9, 2, 2, 6, 0], [22, 4, -2.9, 2, 2, 7.2, 0]
    fr = _calib_frame([far], [0.9], [near, far])
    heights = cref.prepare([fr])[0]["gt_height"]
    assert 55 < heights[0] < 70 and 25 + 1e-2 < heights[1] < 40 - 1e-2
    got, *_ = _compute([fr], metrics=("BEV", "3D"))
    assert got["KITTI/Car_BEV_AP11_easy_strict"] == 0.0          # its detection is too short for easy: flag 1
    assert abs(got["KITTI/Car_BEV_AP11_moderate_strict"] - 100.0 / 11.0) < 1e-9
    assert got["KITTI/Car_BEV_AP11_easy_strict"] != got["KITTI/Car_BEV_AP11_moderate_strict"]
    want = cref.result_dict(cref.evaluate(cref.prepare([fr]), ["Car"], ("BEV", "3D")), ["Car"], ("BEV", "3D"))
    assert set(got) == set(want) and max(abs(got[k] - want[k]) for k in want) < 1e-9


def test_invalid_detections_are_removed_from_every_metric():
    """A detection outside pcd_limit_range on a ground truth outside it: no true positive, no false positive."""
    in_gt, out_gt = [10, 0, -2.95, 2, 4, 2.9, 0], [75, 0, -1, 4, 2, 20, 0]      # 32 px and 27 px high
    fr = _calib_frame([in_gt, out_gt, [10, 30, -3.5, 2, 4, 2, 0]], [0.9, 0.8, 0.7], [in_gt, out_gt])
    got, counts, nthr, detail = _compute([fr])
    assert detail["calib"]["valid"].tolist() == [True, False, False]
    assert (detail["flag_det"][:, 1:] == -1).all()
    for fam in range(3):
        assert counts[fam * 6 + 4, 0].tolist() == [1, 0, 1]     # hard, strict: the far ground truth is a miss
    assert nthr[4] == 1
    _, c_wide, n_wide, d_wide = _compute([fr], pcd_limit_range=(0, -40, -3, 100, 40, 0.0))
    assert d_wide["calib"]["valid"].tolist() == [True, True, False]      # inside the wider range it is a true positive
    assert n_wide[4] == 2 and c_wide[4, 1].tolist() == [2, 0, 0]


def test_cpu_path_equals_the_reference_on_random_frames():
    frames = cc.eval_frames()[0][:10]
    m = ke.KittiAP(cc.CLASSES, metrics=FOUR)
    m.update(*cc.to_update(frames))
    detail = {}
    counts, nthr = m._counts(detail=detail)
    want = cref.evaluate(cref.prepare(frames), cc.CLASSES)
    cc.assert_equal_to_reference(counts, nthr, detail, want, detail["families"])
    got, exp = m.compute(), cref.result_dict(want, cc.CLASSES)
    assert set(got) == set(exp) and max(abs(got[k] - exp[k]) for k in exp) < 1e-9
    assert sum(c[0] for (mm, *_), r in want.items() if mm == "2D" for c in r["counts"]) > 50


# ----------------------------------------------------------------------------------- the margins of the GPU cases
def test_margins_of_the_gpu_cases():
    pc = cc.project_case()
    assert pc["share"] <= cc.MAX_SHARE and pc["off"][-1] == sum(cc.PROJECT_COUNTS) and len(pc["boxes"]) == pc["off"][-1] + 3
    finite = np.isfinite(pc["boxes"][:pc["off"][-1]]).all(1)
    assert (~finite).sum() == 2
    ws = np.array([p["w"] for p in pc["p64"]])[finite]
    assert np.abs(ws).min() >= cc.MIN_W
    assert ((ws < 0).any(1) & (ws > 0).any(1)).sum() >= 10            # boxes across the camera plane
    valid = np.array([p["valid"] for p in pc["p64"]])
    assert 0.3 < valid.mean() < 0.9
    for k, p in enumerate(pc["p64"]):
        if not finite[k]:
            assert not p["valid"]
            continue
        h, w = pc["hws"][pc["rows"][k]]
        r = p["raw"]
        assert min(abs(r[0] - w), abs(r[1] - h), abs(r[2]), abs(r[3])) >= cc.PX
        assert min(abs(p["height"] - 25), abs(p["height"] - 40)) >= cc.PX
        assert min(abs(float(pc["boxes"][k][a]) - f) for a, f in zip((0, 1, 2, 0, 1, 2), cc.RANGE)) >= cc.METRE
        # the float32 restatement decides as float64 does
        r32 = pc["p32"]["raw"][k]
        assert (r32[0] < w, r32[1] < h, r32[2] > 0, r32[3] > 0) == (r[0] < w, r[1] < h, r[2] > 0, r[3] > 0)
    m2d, m3d = cc.overlap_bound_2d(), cc.overlap_bound_3d()
    assert 1e-8 < m2d < 1e-4 and 1e-7 < m3d < 1e-3
    dc = cc.dc_case()
    assert dc["share"] <= cc.MAX_SHARE and 0 < dc["ref_err"] < 1e-5 and 0.05 < dc["want"].mean() < 0.95
    frames, share = cc.eval_frames()
    assert share <= cc.MAX_SHARE and 36 <= len(frames) <= 45
    assert 500 <= len(frames[-1]["det_scores"]) <= 512 and 125 <= len(frames[-1]["gt_labels"]) <= 128
    assert len(frames[-1]["dontcare"]) == 64
    for fr in frames:
        pr = cref.prepare([fr])[0]
        ov = cref.iou_matrix(pr["det_box2d"], pr["gt_box2d"])
        for v in cc.STRICT_VALUES:
            assert ov.size == 0 or np.abs(ov - float(np.float32(v))).min() >= m2d
        if "dontcare" in fr and len(pr["det_box2d"]):
            ratio = cref.dc_matrix(pr["det_box2d"], fr["dontcare"]).max(1)
            for v in cc.STRICT_VALUES:
                assert np.abs(ratio - float(np.float32(v))).min() >= m2d
