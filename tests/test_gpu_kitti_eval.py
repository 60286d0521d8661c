"""KITTI BEV / 3D average precision on the device (csrc/kitti_eval.hip through robustpointclouds_amd/kitti_eval.py,
evaluate.py) against the float64 restatement of the specification, tests/_kitti_eval_ref.py."""
import functools

import numpy as np
import pytest
import torch

from tests import _kitti_eval_cases as cs
from tests import _kitti_eval_ref as kref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------- overlaps
@functools.lru_cache(maxsize=None)
def _overlap_case():
    """The five frames of OVERLAP_SHAPES, then one frame of one pair per row of the degenerate table.
    -> dets, det_off, gts, gt_off, per mode (float64 reference, float32 reference) flat in the product's order,
    number of elements of the five frames, the table's expected values."""
    frames = cs.overlap_frames()
    a, b, want_bev, want_3d = cs.degenerate_pairs7()
    frames += [(b[k:k + 1], a[k:k + 1]) for k in range(len(a))]     # det = b, gt = a: a is the clipper's box
    det_off = np.cumsum([0] + [len(d) for d, _ in frames]).tolist()
    gt_off = np.cumsum([0] + [len(g) for _, g in frames]).tolist()
    refs = {}
    for mode in range(2):
        refs[mode] = tuple(np.concatenate([kref.overlap_matrix(d, g, mode, dt).reshape(-1) for d, g in frames])
                           for dt in (np.float64, np.float32))
    n5 = sum(len(d) * len(g) for d, g in frames[:5])
    return (np.concatenate([d for d, _ in frames]), det_off, np.concatenate([g for _, g in frames]), gt_off, refs, n5,
            (want_bev, want_3d))


@pytest.mark.parametrize("mode", [0, 1])
def test_box_overlaps(mode):
    """F = 5 frames of (Nd, Ng) = (0, 7), (9, 0), (1, 1), (65, 33), (512, 128) — the empty sides, one pair, a
    wave and tile boundary, both caps — about half of the pairs overlapping, plus the degenerate table. The
    bound is 4 x the float32 restatement's own maximum error against float64 on these pairs (operation order,
    fused multiply-adds), per mode. Measured on the MI355X: BEV 2.42e-7 against a bound of 5.48e-5, 3D 2.20e-7
    against 5.50e-5 (the reference's fp32 error is the 1e-3 m slivers of the degenerate table)."""
    from robustpointclouds_amd import kitti_eval as ke
    dets, det_off, gts, gt_off, refs, n5, wants = _overlap_case()
    f64, f32 = refs[mode]
    assert cs.OVERLAP_SHAPES == [(0, 7), (9, 0), (1, 1), (65, 33), (512, 128)] and n5 == 1 + 65 * 33 + 512 * 128
    assert 0.4 < (f64[:n5] > 0).mean() < 0.6
    ref_err = np.abs(f32.astype(np.float64) - f64).max()
    bound = 4.0 * ref_err
    ov, ov_off = ke.box_overlaps(_dev(dets), det_off, _dev(gts), gt_off, mode)
    got = ov.cpu().numpy()
    assert got.shape == f64.shape and ov_off[5] == n5
    err = np.abs(got.astype(np.float64) - f64).max()
    print(f"mode {mode}: fp32 reference error {ref_err:.3e}, bound {bound:.3e}, kernel error {err:.3e}")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    assert 1e-7 < ref_err < 1e-4            # the reference itself is a sane fp32 yardstick
    assert err <= bound
    for g, w in zip(got[n5:], wants[mode]):
        if w in (0.0, 1.0):
            assert g == w                   # identical: exactly 1; touching, disjoint or degenerate: exactly 0


def test_box_overlaps_identical_and_extreme():
    from robustpointclouds_amd import kitti_eval as ke
    dets, gts = cs.overlap_frames()[3]
    same = _dev(dets)
    off = [0, len(dets)]
    for mode in range(2):
        ov, _ = ke.box_overlaps(same, off, same, off, mode)
        assert (ov.view(len(dets), len(dets)).diagonal() == 1.0).all()
    a, b = cs.extreme_pairs7()
    off = list(range(len(a) + 1))
    for mode in range(2):
        for x, y in ((a, b), (b, a)):
            got = ke.box_overlaps(_dev(x), off, _dev(y), off, mode)[0].cpu().numpy()
            assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0


# ----------------------------------------------------------------------------------- matcher, exact
@functools.lru_cache(maxsize=None)
def _frames():
    """About 40 frames: the matcher's branch frames, 30 random ones and the frame at the caps."""
    return list(cs.branch_frames().values()) + cs.random_frames(30, seed=0)


def _metric(frames):
    from robustpointclouds_amd import kitti_eval as ke
    m = ke.KittiAP(cs.CLASSES)
    m.update(*cs.to_update(frames, DEV))
    return m


def test_matcher_is_exact_on_the_devices_own_overlaps():
    """The reference loops fed the DEVICE's fp32 overlap matrices and the fp32 scores: pass-1 scores, thresholds
    and every tp / fp / fn at every threshold are equal, no tolerance — all classes x difficulties x tables x
    both metrics, flags of all three values, the (512, 128) frame included. Twice: bit-identical."""
    frames = _frames()
    assert 38 <= len(frames) <= 45 and frames[-1]["det_boxes"].shape[0] == 512 and frames[-1]["gt_boxes"].shape[0] == 128
    m = _metric(frames)
    counts, nthr, detail = cs.product_detail(m)
    assert detail["overlaps"][0].is_cuda and detail["tp_scores"].is_cuda
    want = kref.evaluate(frames, cs.CLASSES, overlaps=cs.frame_overlaps(detail))
    cs.assert_equal_to_reference(counts, nthr, detail, want)
    fd, fg = detail["flag_det"].cpu().numpy(), detail["flag_gt"].cpu().numpy()
    for row in range(9):
        assert set(np.unique(fd[row])) == {-1, 0, 1} and set(np.unique(fg[row])) == {-1, 0, 1}
    assert max(nthr) > 20 and min(nthr) < max(nthr)
    assert sum(c[0] for r in want.values() for c in r["counts"]) > 1000
    counts2, nthr2, detail2 = cs.product_detail(m)
    assert nthr2 == nthr and torch.equal(counts2, counts)
    assert torch.equal(detail2["tp_scores"], detail["tp_scores"]) and torch.equal(detail2["thr"], detail["thr"])


def test_end_to_end_against_float64():
    """Detections with a float64 overlap within the overlap bound of a table value are dropped (at most 2 %);
    the counts then equal the all-float64 reference and every AP agrees to 1e-9."""
    refs = _overlap_case()[4]     # the margin is the overlap bound of test_box_overlaps, the larger of the two modes
    margin = 4.0 * max(np.abs(f32.astype(np.float64) - f64).max() for f64, f32 in refs.values())
    frames, share, _ = cs.drop_ambiguous(_frames(), margin)
    print(f"margin {margin:.3e}, share of detections dropped {share:.4f}")
    assert share <= 0.02
    m = _metric(frames)
    counts, nthr, detail = cs.product_detail(m)
    want = kref.evaluate(frames, cs.CLASSES)
    cs.assert_equal_to_reference(counts, nthr, detail, want)
    got, exp = m.compute(), kref.result_dict(want, cs.CLASSES)
    assert set(got) == set(exp)
    for k in exp:
        assert abs(got[k] - exp[k]) <= 1e-9, (k, got[k], exp[k])
    assert 1.0 < got["KITTI/Car_BEV_AP40_moderate_strict"] < 100.0


@pytest.mark.parametrize("case, ap11, ap40, nthr", [(cs.hand_single, 100.0 / 11.0, 0.0, 1), (cs.hand_41, 100.0, 100.0, 41),
                                                    (cs.hand_40_interleaved, 500.0 / 11.0, 48.75, 40)])
def test_hand_values_on_the_device(case, ap11, ap40, nthr):
    """The hand values of tests/test_kitti_eval_cpu.py through the kernels; hand_41 uses all 41 threshold lanes."""
    m = _metric(case())
    counts, nt, detail = cs.product_detail(m)
    assert detail["overlaps"][1].is_cuda and nt[0] == nthr
    got = m.compute()
    for metric in ("BEV", "3D"):
        assert abs(got[f"KITTI/Car_{metric}_AP11_hard_strict"] - ap11) <= 1e-9
        assert abs(got[f"KITTI/Car_{metric}_AP40_easy_loose"] - ap40) <= 1e-9


# ----------------------------------------------------------------------------------- argument errors
def test_argument_errors_return_before_any_launch():
    from robustpointclouds_amd import _ffi
    from robustpointclouds_amd import kitti_eval as ke
    lib = _ffi.load()
    assert (_ffi.KITTI_MAX_DET, _ffi.KITTI_MAX_GT, _ffi.KITTI_MAX_THR) == (512, 128, 41)
    z = torch.zeros(64, dtype=torch.float32, device=DEV)
    off = torch.zeros(2, dtype=torch.int32, device=DEV)
    off64 = torch.zeros(2, dtype=torch.int64, device=DEV)
    p = _ffi.ptr
    ok = lambda *a: lib.rpc_kitti_overlaps(*a, None)
    assert ok(p(z), p(off), p(z), p(off), p(off64), 1, 1, 1, 0, p(z)) == 0          # a frame of nothing
    assert ok(p(z), p(off), p(z), p(off), p(off64), 1, 513, 1, 0, p(z)) != 0        # above the caps
    assert ok(p(z), p(off), p(z), p(off), p(off64), 1, 1, 129, 0, p(z)) != 0
    assert ok(p(z), p(off), p(z), p(off), p(off64), -1, 1, 1, 0, p(z)) != 0         # negative counts
    assert ok(p(z), p(off), p(z), p(off), p(off64), 1, -1, 1, 0, p(z)) != 0
    assert ok(p(z), p(off), p(z), p(off), p(off64), 1, 1, 1, 2, p(z)) != 0          # no such mode
    assert ok(None, p(off), p(z), p(off), p(off64), 1, 1, 1, 0, p(z)) != 0          # null pointers
    assert ok(p(z), None, p(z), p(off), p(off64), 1, 1, 1, 0, p(z)) != 0
    assert ok(p(z), p(off), p(z), p(off), None, 1, 1, 1, 0, p(z)) != 0
    assert ok(p(z), p(off), p(z), p(off), p(off64), 1, 1, 1, 0, None) != 0
    flags = torch.zeros(64, dtype=torch.int8, device=DEV)
    cnt = torch.zeros(41 * 3, dtype=torch.int32, device=DEV)
    nthr = torch.zeros(1, dtype=torch.int32, device=DEV)
    head = (p(z), p(off64), p(off), p(off))
    tail = (p(z), p(flags), p(flags), 1, 1, p(z), 1, 1)
    assert lib.rpc_kitti_match_scores(*head, 1, 1, 1, *tail, p(z), None) == 0
    assert lib.rpc_kitti_match_scores(*head, 1, 513, 1, *tail, p(z), None) != 0
    assert lib.rpc_kitti_match_scores(*head, 1, 1, 1, *tail, None, None) != 0
    assert lib.rpc_kitti_match_scores(*head, 1, 1, 1, p(z), None, p(flags), 1, 1, p(z), 1, 1, p(z), None) != 0
    assert lib.rpc_kitti_match_scores(*head, 1, 1, 1, p(z), p(flags), p(flags), 1, 1, p(z), 3, 2, p(z), None) != 0
    assert lib.rpc_kitti_match_counts(*head, 1, 1, 1, *tail, p(z), p(nthr), p(cnt), None) == 0
    assert lib.rpc_kitti_match_counts(*head, 1, 1, 129, *tail, p(z), p(nthr), p(cnt), None) != 0
    assert lib.rpc_kitti_match_counts(*head, 1, 1, 1, *tail, None, p(nthr), p(cnt), None) != 0
    assert lib.rpc_kitti_match_counts(*head, 1, 1, 1, *tail, p(z), p(nthr), None, None) != 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ke.box_overlaps(torch.zeros(513, 7, device=DEV), [0, 513], torch.zeros(1, 7, device=DEV), [0, 1], 0)
    with pytest.raises(ValueError):
        ke.box_overlaps(torch.zeros(1, 7, device=DEV), [0, 1], torch.zeros(129, 7, device=DEV), [0, 129], 1)
    m = ke.KittiAP(cs.CLASSES)
    with pytest.raises(ValueError):
        m.update([dict(bboxes_3d=torch.zeros(513, 7, device=DEV), scores_3d=torch.zeros(513, device=DEV),
                       labels_3d=torch.zeros(513, dtype=torch.int64, device=DEV))],
                 [dict(bboxes_3d=torch.zeros(0, 7), labels_3d=torch.zeros(0, dtype=torch.int64))])


# ----------------------------------------------------------------------------------- robustness_report
def test_robustness_report_on_the_synthetic_voxelnet():
    """The smallest synthetic AdversarialVoxelNet of tests/test_gpu_predict_eval.py: complete keys, values in
    [0, 100], the clean result equal to KittiAP fed the same `predict` output by hand, buffers unchanged."""
    from robustpointclouds_amd import kitti_eval as ke
    from robustpointclouds_amd import robustness_report
    from robustpointclouds_amd.synthetic import kitti_batch
    from tests.test_gpu_predict_eval import _buffers, _data, _model, _same_bytes
    model = _model()
    pts, boxes, labels = kitti_batch(2, seed0=21, num_classes=3)
    frames = [p[::4] for p in pts]
    gts = [dict(bboxes_3d=torch.from_numpy(np.asarray(b, dtype=np.float32)).reshape(-1, 7),
                labels_3d=torch.from_numpy(np.asarray(l, dtype=np.int64)).reshape(-1)) for b, l in zip(boxes, labels)]
    batches = [(_data(frames[:1]), gts[:1]), (_data(frames[1:]), gts[1:])]
    before = _buffers(model)
    modes = {n: m.training for n, m in model.named_modules()}
    rep = robustness_report(model, batches, cs.CLASSES)
    torch.cuda.synchronize()
    after = _buffers(model)
    assert set(after) == set(before) and all(_same_bytes(before[k], after[k]) for k in before)
    assert {n: m.training for n, m in model.named_modules()} == modes and model._attack_eval is False
    keys = {f"KITTI/{c}_{m}_AP{r}_{d}_{t}" for c in cs.CLASSES for m in ("BEV", "3D") for r in (11, 40)
            for d in ("easy", "moderate", "hard") for t in ("strict", "loose")}
    keys |= {f"KITTI/Overall_{m}_AP{r}_{d}" for m in ("BEV", "3D") for r in (11, 40) for d in ("easy", "moderate", "hard")}
    assert set(rep) == {"clean", "attacked", "drop"}
    for part in ("clean", "attacked"):
        assert set(rep[part]) == keys
        assert all(isinstance(v, float) and 0.0 <= v <= 100.0 for v in rep[part].values())
    assert all(rep["drop"][k] == rep["clean"][k] - rep["attacked"][k] for k in keys)
    by_hand = ke.KittiAP(cs.CLASSES)
    for data, g in batches:
        preds = model.val_step(data)
        assert preds[0]["bboxes_3d"].is_cuda
        by_hand.update(preds, g)
    assert by_hand.compute() == rep["clean"]
