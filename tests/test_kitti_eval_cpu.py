"""KITTI BEV / 3D average precision on the CPU path (robustpointclouds_amd/kitti_eval.py) against the float64
restatement of the specification (tests/_kitti_eval_ref.py), and evaluate / robustness_report on a stub model.
The HIP kernels are covered by tests/test_gpu_kitti_eval.py."""
import contextlib

import numpy as np
import pytest
import torch
from torch import nn

from robustpointclouds_amd import evaluate, robustness_report
from robustpointclouds_amd import kitti_eval as ke
from tests import _kitti_eval_cases as cs
from tests import _kitti_eval_ref as kref

CAR = (0, 0, 0, 0)   # BEV, Car, easy, strict


def _product(frames, classes=cs.CLASSES):
    m = ke.KittiAP(classes)
    m.update(*cs.to_update(frames))
    return m


def _check(frames, classes=cs.CLASSES):
    """The CPU path equals the reference on these frames: intermediate results exactly, every AP to 1e-9."""
    m = _product(frames, classes)
    want = kref.evaluate(frames, classes)
    counts, nthr, detail = cs.product_detail(m)
    ref_ov = {mode: [kref.overlap_matrix(f["det_boxes"], f["gt_boxes"], mode) for f in frames] for mode in range(2)}
    for mode, per_frame in cs.frame_overlaps(detail).items():
        for got, exp in zip(per_frame, ref_ov[mode]):
            assert got.shape == exp.shape and (np.abs(got - exp).max() if got.size else 0.0) <= 1e-6
    cs.assert_equal_to_reference(counts, nthr, detail, want, len(classes))
    got, exp = m.compute(), kref.result_dict(want, classes)
    assert set(got) == set(exp)
    for k in exp:
        assert isinstance(got[k], float) and abs(got[k] - exp[k]) <= 1e-9, (k, got[k], exp[k])
    return got, want


# ----------------------------------------------------------------------------------- hand values
@pytest.mark.parametrize("case, ap11, ap40, nthr", [(cs.hand_single, 100.0 / 11.0, 0.0, 1), (cs.hand_41, 100.0, 100.0, 41),
                                                    (cs.hand_40_interleaved, 500.0 / 11.0, 48.75, 40)])
def test_hand_values(case, ap11, ap40, nthr):
    frames = case()
    got, want = _check(frames)
    assert len(want[CAR]["thresholds"]) == nthr
    for metric in ("BEV", "3D"):
        for diff in ke.DIFFICULTIES:       # no difficulty fields: the three coincide
            for table in ("strict", "loose"):
                assert abs(got[f"KITTI/Car_{metric}_AP11_{diff}_{table}"] - ap11) <= 1e-9
                assert abs(got[f"KITTI/Car_{metric}_AP40_{diff}_{table}"] - ap40) <= 1e-9
            # the other classes have nothing: Overall is the mean over the three classes of the strict values
            assert abs(got[f"KITTI/Overall_{metric}_AP11_{diff}"] - ap11 / 3.0) <= 1e-9
    assert got["KITTI/Pedestrian_3D_AP40_moderate_strict"] == 0.0


def test_result_keys_are_complete():
    got = _product(cs.hand_single()).compute()
    keys = {f"KITTI/{c}_{m}_AP{r}_{d}_{t}" for c in cs.CLASSES for m in ("BEV", "3D") for r in (11, 40)
            for d in ("easy", "moderate", "hard") for t in ("strict", "loose")}
    keys |= {f"KITTI/Overall_{m}_AP{r}_{d}" for m in ("BEV", "3D") for r in (11, 40) for d in ("easy", "moderate", "hard")}
    assert set(got) == keys and all(0.0 <= v <= 100.0 for v in got.values())


# ----------------------------------------------------------------------------------- the matcher's branches
BRANCH_WANT = {   # name -> {(mode, class, difficulty, table): (thresholds, counts)}
    "equal_scores": {CAR: ([0.5], [(1, 1, 0)])},
    "neighbour_absorbs": {CAR: ([0.8], [(1, 0, 0)])},
    "took_ignored": {CAR: ([0.9, 0.5], [(1, 0, 1), (2, 0, 0)]), (1, 0, 1, 0): ([0.9, 0.5], [(1, 0, 1), (2, 0, 0)])},
    "short_other_class": {CAR: ([0.8], [(1, 0, 0)]), (0, 1, 0, 0): ([], [])},
    "below_threshold": {CAR: ([0.9, 0.3], [(1, 0, 1), (2, 0, 0)])},
    "class_without_gt": {CAR: ([0.9], [(1, 0, 0)]), (0, 2, 0, 0): ([], []), (1, 2, 2, 1): ([], [])},
    "empty": {CAR: ([], [])},
    "only_dets": {CAR: ([], [])},
    "only_gts": {CAR: ([], [])},
    "difficulty": {CAR: ([0.8], [(1, 0, 0)]), (0, 0, 2, 0): ([0.9, 0.8], [(1, 0, 1), (2, 0, 0)])},
}


@pytest.mark.parametrize("name", sorted(BRANCH_WANT))
def test_matcher_branch(name):
    """One small frame per branch of the matcher: the values worked out by hand in _kitti_eval_cases.branch_frames
    hold for the reference, and the CPU path equals the reference in every group."""
    fr = cs.branch_frames()[name]
    got, want = _check([fr])
    f32 = lambda v: [float(np.float32(x)) for x in v]
    for key, (thr, counts) in BRANCH_WANT[name].items():
        assert want[key]["thresholds"] == f32(thr), (key, want[key]["thresholds"])
        assert want[key]["counts"] == counts, (key, want[key]["counts"])
    if name == "equal_scores":
        assert want[CAR]["tp_scores"] == [[(0, 0.5)]]
    if name == "class_without_gt":
        assert all(v == 0.0 for k, v in got.items() if "Cyclist" in k)
    if name in ("empty", "only_dets", "only_gts"):
        assert all(v == 0.0 for v in got.values())


def test_all_branch_frames_together_and_fewer_than_41_thresholds():
    frames = list(cs.branch_frames().values())
    got, want = _check(frames)
    assert 1 < len(want[CAR]["thresholds"]) < 41
    assert 0.0 < got["KITTI/Car_BEV_AP11_easy_strict"] < 100.0


def test_random_frames_equal_the_reference():
    frames = cs.random_frames(6, seed=1, cap_frame=False)
    got, want = _check(frames)
    flags = set()
    for fr in frames:
        for l, h in zip(fr["det_labels"], fr["det_height"]):
            flags.add(("d", kref.det_flag(int(l), float(h), 0, 0)))
        for l, nb, h, o, t in zip(fr["gt_labels"], fr["gt_neighbor"], fr["gt_height"], fr["gt_occluded"],
                                  fr["gt_truncated"]):
            flags.add(("g", kref.gt_flag(int(l), int(nb), float(h), float(o), float(t), 0, 0)))
    assert flags == {(s, v) for s in "dg" for v in (-1, 0, 1)}
    assert any(len(r["thresholds"]) > 3 for r in want.values())


def test_threshold_positions_jump_equals_the_scan():
    """threshold_indices finds each threshold by a jump and a short walk; the reference scans every score."""
    r = np.random.RandomState(0)
    cases = [(1, 1), (1, 5), (5, 5), (41, 41), (40, 41), (3, 1000), (999, 1000), (1000, 1000), (45228, 45228)]
    cases += [(int(a), int(a + b)) for a, b in zip(r.randint(1, 3000, 40), r.randint(0, 3000, 40))]
    for n_scores, n_valid in cases:
        scores = list(range(n_scores, 0, -1))     # descending, distinct: the score is its position from the end
        want = [n_scores - s for s in kref.thresholds(scores, n_valid)]
        assert ke.threshold_indices(n_scores, n_valid) == want, (n_scores, n_valid)
        assert len(want) <= 41
    assert ke.threshold_indices(0, 5) == [] and ke.threshold_indices(5, 0) == []


def test_min_overlaps_and_caps():
    with pytest.raises(ValueError):
        ke.KittiAP(["Car", "Truck"])
    m = ke.KittiAP(["Truck"], min_overlaps={"Truck": (0.7, 0.5)})
    m.update(*cs.to_update(cs.hand_single()))
    assert abs(m.compute()["KITTI/Truck_3D_AP11_easy_strict"] - 100.0 / 11.0) <= 1e-9
    m.reset()
    assert len(m) == 0 and all(v == 0.0 for v in m.compute().values())
    big = cs.frame([cs.box(k, 0) for k in range(513)], [0.5] * 513, [0] * 513)
    with pytest.raises(ValueError):
        m.update(*cs.to_update([big]))
    big = cs.frame(gt_boxes=[cs.box(k, 0) for k in range(129)], gt_labels=[0] * 129)
    with pytest.raises(ValueError):
        m.update(*cs.to_update([big]))
    with pytest.raises(ValueError):
        ke.box_overlaps(torch.zeros(513, 7), [0, 513], torch.zeros(1, 7), [0, 1], 0)


def test_box_overlaps_cpu_degenerate_table():
    a, b, want_bev, want_3d = cs.degenerate_pairs7()
    n = len(a)
    off = list(range(n + 1))
    for mode, want in ((0, want_bev), (1, want_3d)):
        ov, ov_off = ke.box_overlaps(torch.from_numpy(b), off, torch.from_numpy(a), off, mode)
        assert ov.dtype == torch.float32 and ov_off == off
        for k, w in enumerate(want):
            exp = float(kref.overlap(a[k], b[k], mode))
            assert abs(float(ov[k]) - exp) <= 1e-6
            if w in (0.0, 1.0):
                assert float(ov[k]) == w, (mode, k)
    # 9-column boxes: the first 7 columns count
    a9 = torch.cat([torch.from_numpy(a), torch.ones(n, 2)], 1)
    ov9, _ = ke.box_overlaps(a9, off, a9, off, 1)
    ov7, _ = ke.box_overlaps(torch.from_numpy(a), off, torch.from_numpy(a), off, 1)
    assert torch.equal(ov9, ov7)


def test_reference_array_form_equals_its_loops():
    """The reference's overlap on arrays (what the tests use for whole matrices) against its plain loops."""
    dets, gts = cs.overlap_frames()[3]
    a, b, _, _ = cs.degenerate_pairs7()
    a, b = np.concatenate([np.tile(gts, (4, 1)), a]), np.concatenate([np.repeat(dets[:4], len(gts), 0), b])
    for mode in range(2):
        for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-6)):
            vec = kref.overlap_pairs(a, b, mode, dtype)
            loop = np.array([kref.overlap(x, y, mode, dtype) for x, y in zip(a, b)])
            assert vec.dtype == dtype and np.abs(vec.astype(np.float64) - loop.astype(np.float64)).max() <= tol
            assert (vec > 0).sum() > 40


# ----------------------------------------------------------------------------------- evaluate / robustness_report
class StubDetector(nn.Module):
    """val_step returns the detections stored in the batch; inside attack_eval() only every second one."""

    def __init__(self):
        super().__init__()
        self.body = nn.Linear(2, 2)
        self.frozen = nn.BatchNorm1d(2)
        self._attack_eval = False
        self.calls = []

    @contextlib.contextmanager
    def attack_eval(self):
        prev, self._attack_eval = self._attack_eval, True
        try:
            yield self
        finally:
            self._attack_eval = prev

    def val_step(self, data):
        self.calls.append((self._attack_eval, self.training, self.body.training, self.frozen.training))
        if data.get("raise"):
            raise ZeroDivisionError
        preds = data["preds"]
        if self._attack_eval:
            preds = [{k: v[::2] for k, v in p.items()} for p in preds]
        return preds


def _batches():
    frames = list(cs.branch_frames().values()) + cs.hand_41()
    out = []
    for k in range(0, len(frames), 3):
        preds, gts = cs.to_update(frames[k:k + 3])
        out.append((dict(preds=preds), gts))
    return frames, out


def test_evaluate_and_robustness_report_on_a_stub():
    frames, batches = _batches()
    model = StubDetector().train()
    model.frozen.eval()                     # a module with a mode of its own
    rep = robustness_report(model, batches, cs.CLASSES)
    n = len(batches)
    # the clean run outside, the attacked run inside attack_eval; the whole model in eval mode both times
    assert model.calls == [(False, False, False, False)] * n + [(True, False, False, False)] * n
    assert model.training and model.body.training and not model.frozen.training and model._attack_eval is False
    want = kref.result_dict(kref.evaluate(frames, cs.CLASSES), cs.CLASSES)
    half = [dict(f, **{k: f[k][::2] for k in ("det_boxes", "det_scores", "det_labels", "det_height")}) for f in frames]
    want_att = kref.result_dict(kref.evaluate(half, cs.CLASSES), cs.CLASSES)
    assert set(rep) == {"clean", "attacked", "drop"}
    for k in want:
        assert abs(rep["clean"][k] - want[k]) <= 1e-9 and abs(rep["attacked"][k] - want_att[k]) <= 1e-9
        assert rep["drop"][k] == rep["clean"][k] - rep["attacked"][k]
    assert rep["drop"]["KITTI/Car_3D_AP40_easy_strict"] > 0.0
    # evaluate alone, with a metric that already holds frames: it is reset first
    metric = ke.KittiAP(cs.CLASSES)
    metric.update(*cs.to_update(cs.hand_single()))
    assert evaluate(model.eval(), batches, metric) == rep["clean"]
    assert not model.training


def test_evaluate_restores_the_mode_when_a_batch_raises_and_refuses_models_without_attack_eval():
    _, batches = _batches()
    model = StubDetector().train()
    with pytest.raises(ZeroDivisionError):
        evaluate(model, batches[:1] + [(dict(raise_=True, **{"raise": True}), [])], ke.KittiAP(cs.CLASSES), attacked=True)
    assert model.training and model.body.training and model._attack_eval is False

    class Plain(nn.Module):
        def val_step(self, data):
            return data["preds"]

    with pytest.raises(TypeError):
        evaluate(Plain(), batches, ke.KittiAP(cs.CLASSES), attacked=True)
    clean = evaluate(Plain(), batches, ke.KittiAP(cs.CLASSES))
    assert clean["KITTI/Car_BEV_AP11_easy_strict"] > 0.0
