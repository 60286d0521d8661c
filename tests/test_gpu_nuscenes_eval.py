"""nuScenes detection score on the device (csrc/nuscenes_eval.hip through robustpointclouds_amd/nuscenes_eval.py,
evaluate.py) against the float64 restatement of the specification, tests/_nuscenes_eval_ref.py, on the inputs of
tests/_nuscenes_eval_cases.py (float32 takes float64's decisions on them: tests/test_nuscenes_eval_cpu.py)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import _nuscenes_eval_cases as cs
from tests import _nuscenes_eval_ref as nref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ARITH = ("trans", "scale", "orient", "vel")     # the error columns that are arithmetic; attr is a comparison


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _frames():
    """The branch frames, 30 random ones and the shape frames, the one at the caps (500, 512) last."""
    return list(cs.branch_frames().values()) + cs.random_frames(30, seed=0) + cs.shape_frames()


@functools.lru_cache(maxsize=None)
def _ref():
    return nref.evaluate(_frames(), cs.CLASSES)


@functools.lru_cache(maxsize=None)
def _bounds():
    """Per arithmetic error column: 4 x the float32 reference's own maximum error against float64 on these
    matches (operation order, fused multiply-adds). -> ({column: bound}, {column: fp32 reference error})."""
    r64 = _ref()
    r32 = nref.evaluate(_frames(), cs.CLASSES, dtype=np.float32, scores=False)
    assert np.array_equal(r32["match"], r64["match"])
    ref_err = {m: float(np.abs(np.nan_to_num(r32["err"][:, k] - r64["err"][:, k])).max()) for k, m in enumerate(ARITH)}
    return {m: 4.0 * e for m, e in ref_err.items()}, ref_err


def _metric(frames, device=DEV):
    from robustpointclouds_amd import nuscenes_eval as ne
    m = ne.NuScenesDetectionScore()
    m.update(*cs.to_update(frames, device))
    return m


def _center_matches(frames, ref, thresholds=None):
    from robustpointclouds_amd import nuscenes_eval as ne
    flat = cs.flat_inputs(frames, ref)
    args = [_dev(flat["det_xy"]), _dev(flat["det_label"]), _dev(flat["det_keep"]), flat["det_off"], _dev(flat["gt_xy"]),
            _dev(flat["gt_label"]), _dev(flat["gt_keep"]), flat["gt_off"], 10]
    got = ne.center_matches(*args) if thresholds is None else ne.center_matches(*args, thresholds)
    assert got.is_cuda and got.dtype == torch.int32
    return got.cpu().numpy(), ref["match"][:, flat["perm"]]


# ----------------------------------------------------------------------------------- rpc_nus_match, exact
def test_match_kernel_equals_the_reference():
    """All frames in one call: every threshold's matches equal the reference's, no tolerance — (0, 5), (7, 0),
    (1, 1), (65, 33) and (500, 512) included, filtered boxes and labels of -1 among them. Then the frames in
    reversed order (the ragged offsets), and eight thresholds (RPC_NUS_MAX_THR)."""
    frames, ref = _frames(), _ref()
    assert 45 <= len(frames) <= 60 and frames[-1]["det_boxes"].shape[0] == 500 and frames[-1]["gt_boxes"].shape[0] == 512
    got, want = _center_matches(frames, ref)
    assert got.shape == want.shape == (4, sum(len(f["det_boxes"]) for f in frames))
    for t in range(4):
        assert np.array_equal(got[t], want[t]), t
    assert (want[2] >= 0).sum() > 500 and (want[0] != want[3]).sum() > 50
    again, _ = _center_matches(frames, ref)
    assert np.array_equal(again, got)
    rev = frames[::-1]
    got, want = _center_matches(rev, nref.evaluate(rev, cs.CLASSES, scores=False))
    assert np.array_equal(got, want)
    ref8 = nref.evaluate(frames, cs.CLASSES, thresholds=cs.EIGHT_THRESHOLDS, scores=False)
    got, want = _center_matches(frames, ref8, cs.EIGHT_THRESHOLDS)
    assert got.shape[0] == 8 and np.array_equal(got, want)
    assert len({tuple(r) for r in want.tolist()}) == 8      # eight different rows


# ----------------------------------------------------------------------------------- rpc_nus_tp_errors
def test_tp_errors_within_the_float32_yardstick():
    """Per error column the bound is 4 x the float32 reference's own maximum error against float64 on these
    matches. attr_err and the NaN pattern are equal exactly.
    Measured on the MI355X (kernel error / fp32 reference error / bound): trans 5.93e-8 / 5.93e-8 / 2.37e-7,
    scale 1.29e-7 / 1.36e-7 / 5.44e-7, orient 1.07e-6 / 1.07e-6 / 4.26e-6, vel 4.59e-7 / 4.59e-7 / 1.84e-6."""
    bounds, ref_err = _bounds()
    ref = _ref()
    m = _metric(_frames())
    match, err, order = m._matches()
    assert np.array_equal(match.numpy(), ref["match"]) and np.array_equal(order.numpy(), ref["order"])
    got = err.numpy()
    assert got.dtype == np.float32 and got.shape == ref["err"].shape
    assert np.array_equal(np.isnan(got), np.isnan(ref["err"]))
    hit = ref["match"][2] >= 0
    assert hit.sum() > 500 and np.isnan(got[~hit]).all() and np.isnan(ref["err"][hit][:, 3:]).any()
    errs = {}
    for k, name in enumerate(ARITH):
        errs[name] = float(np.abs(np.nan_to_num(got[:, k].astype(np.float64) - ref["err"][:, k])).max())
        print(f"{name}_err: kernel error {errs[name]:.3e}, fp32 reference error {ref_err[name]:.3e}, bound {bounds[name]:.3e}")
    for name in ARITH:
        assert 0.0 < ref_err[name] < 1e-5, name           # the reference itself is a sane fp32 yardstick
        assert errs[name] <= bounds[name], name
    a, b = got[:, 4], ref["err"][:, 4]
    assert np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]) and set(np.unique(a[~np.isnan(a)])) == {0.0, 1.0}


# ----------------------------------------------------------------------------------- compute()
def _close(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


def test_compute_on_the_device():
    """AP keys and mAP within 1e-12 of the reference (the same integers and the same fp32 scores); error keys and
    NDS within the largest column bound + 1e-12 (means and interpolation are convex). The device path equals the
    CPU path under the same bounds."""
    bounds, _ = _bounds()
    etol = max(bounds.values()) + 1e-12
    ref = _ref()["result"]
    m = _metric(_frames())
    assert m._det[0][0].is_cuda and m._gt[0][0].is_cuda
    got = m.compute()
    cpu = _metric(_frames(), None).compute()
    assert set(got) == set(ref) == set(cpu) and len(got) == 97
    worst = 0.0
    for k, v in ref.items():
        tol = 1e-12 if ("_AP_" in k or k == "NuScenes/mAP") else etol
        assert _close(got[k], v, tol), (k, got[k], v)
        assert _close(got[k], cpu[k], tol), (k, got[k], cpu[k])
        if not math.isnan(v):
            worst = max(worst, abs(got[k] - v))
    print(f"compute(): largest difference to the reference {worst:.3e} (error-key tolerance {etol:.3e})")
    assert 0.05 < got["NuScenes/mAP"] < 0.95 and 0.0 < got["NuScenes/NDS"] < 1.0
    # an empty metric on the device, and one whose frames hold nothing
    from robustpointclouds_amd import nuscenes_eval as ne
    e = ne.NuScenesDetectionScore()
    e.update([dict(bboxes_3d=torch.zeros(0, 9, device=DEV), scores_3d=torch.zeros(0, device=DEV),
                   labels_3d=torch.zeros(0, dtype=torch.int64, device=DEV))],
             [dict(bboxes_3d=torch.zeros(0, 9), labels_3d=torch.zeros(0, dtype=torch.int64))])
    out = e.compute()
    assert out["NuScenes/NDS"] == 0.0 and out["NuScenes/mAP"] == 0.0 and out["NuScenes/car_trans_err"] == 1.0


# ----------------------------------------------------------------------------------- argument errors
def test_argument_errors_return_before_any_launch():
    from robustpointclouds_amd import _ffi
    from robustpointclouds_amd import nuscenes_eval as ne
    lib = _ffi.load()
    assert (_ffi.NUS_MAX_DET, _ffi.NUS_MAX_GT, _ffi.NUS_MAX_THR) == (512, 512, 8)
    z = torch.zeros(64, dtype=torch.float32, device=DEV)
    lab = torch.zeros(64, dtype=torch.int32, device=DEV)
    keep = torch.ones(64, dtype=torch.int8, device=DEV)
    off = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.full((64,), 7, dtype=torch.int32, device=DEV)
    p = _ffi.ptr
    ARG, UNSUPPORTED = 1, 3

    def match(det_xy=z, det_label=lab, det_keep=keep, det_off=off, gt_xy=z, gt_label=lab, gt_keep=keep, gt_off=off,
              frames=1, max_det=1, max_gt=1, n_det=1, n_gt=1, n_classes=1, thr=z, n_thr=1, res=out):
        t = lambda v: None if v is None else p(v)
        return lib.rpc_nus_match(t(det_xy), t(det_label), t(det_keep), t(det_off), t(gt_xy), t(gt_label), t(gt_keep),
                                 t(gt_off), frames, max_det, max_gt, n_det, n_gt, n_classes, t(thr), n_thr, t(res), None)

    assert match(frames=0) == 0 and match(n_det=0) == 0 and match(n_thr=0) == 0      # successful no-ops
    torch.cuda.synchronize()
    assert (out == 7).all()                                                           # nothing was written
    for name in ("det_xy", "det_label", "det_keep", "det_off", "gt_xy", "gt_label", "gt_keep", "gt_off", "thr", "res"):
        assert match(**{name: None}) == ARG, name
    for name in ("frames", "max_det", "max_gt", "n_det", "n_gt", "n_classes", "n_thr"):
        assert match(**{name: -1}) == ARG, name
    assert match(max_det=513) == UNSUPPORTED and match(max_gt=513) == UNSUPPORTED and match(n_thr=9) == UNSUPPORTED
    assert match(max_det=512, max_gt=512, n_thr=8, n_det=0) == 0

    def errors(det=z, gt=z, m=lab, period=z, da=lab, ga=lab, n_det=1, n_gt=1, res=z):
        t = lambda v: None if v is None else p(v)
        return lib.rpc_nus_tp_errors(t(det), t(gt), t(m), t(period), t(da), t(ga), n_det, n_gt, t(res), None)

    assert errors(n_det=0) == 0
    for name in ("det", "gt", "m", "period", "da", "ga", "res"):
        assert errors(**{name: None}) == ARG, name
    assert errors(n_det=-1) == ARG and errors(n_gt=-1) == ARG
    torch.cuda.synchronize()
    assert (z == 0).all() and (out == 7).all()
    with pytest.raises(ValueError):
        ne.center_matches(torch.zeros(513, 2, device=DEV), torch.zeros(513, device=DEV), torch.ones(513, device=DEV),
                          [0, 513], torch.zeros(1, 2, device=DEV), torch.zeros(1, device=DEV), torch.ones(1, device=DEV),
                          [0, 1], 1)
    m = ne.NuScenesDetectionScore()
    with pytest.raises(ValueError):
        m.update([dict(bboxes_3d=torch.zeros(501, 9, device=DEV), scores_3d=torch.zeros(501, device=DEV),
                       labels_3d=torch.zeros(501, dtype=torch.int64, device=DEV))],
                 [dict(bboxes_3d=torch.zeros(0, 9), labels_3d=torch.zeros(0, dtype=torch.int64))])
    assert len(m) == 0


# ----------------------------------------------------------------------------------- robustness_report
def test_robustness_report_on_the_synthetic_centerpoint():
    """AdversarialCenterPoint (the nuScenes configuration, one-sweep synthetic frames thinned to a quarter) at
    `_epoch = 3`, two batches with ground truth: every key finite or a specified NaN, the clean result identical
    to a second clean run, the attacked run's detections carry perturbation_l2_norm and the clean ones do not, no
    buffer of the checkpoint changed, every module's `training` as before."""
    from robustpointclouds_amd import nuscenes_eval as ne
    from robustpointclouds_amd import robustness_report
    from robustpointclouds_amd.evaluate import evaluate
    from robustpointclouds_amd.synthetic import nus_frame, nus_gt_boxes
    from robustpointclouds_amd.trainer import make_nus_model
    from tests.test_gpu_predict_eval import _buffers, _same_bytes

    class Recording(ne.NuScenesDetectionScore):
        seen = []

        def update(self, preds, gts):
            self.seen.append([p.get("perturbation_l2_norm") for p in preds])
            super().update(preds, gts)

    torch.manual_seed(3)
    model = make_nus_model(device=DEV, epoch=3).eval()
    batches = []
    for i in range(2):
        pts = torch.from_numpy(nus_frame(30 + i, sweeps=1)[::4].copy()).to(DEV)
        boxes, labels = nus_gt_boxes(30 + i)
        batches.append((dict(inputs=dict(points=[pts]), data_samples=None),
                        [dict(bboxes_3d=torch.from_numpy(boxes), labels_3d=torch.from_numpy(labels))]))
    before = _buffers(model)
    modes = {n: m.training for n, m in model.named_modules()}
    metric = Recording()
    rep = robustness_report(model, batches, None, metric=metric)
    torch.cuda.synchronize()
    after = _buffers(model)
    assert set(after) == set(before) and all(_same_bytes(before[k], after[k]) for k in before)
    assert {n: m.training for n, m in model.named_modules()} == modes and model._attack_eval is False
    assert len(metric) == 2 and metric._det[0][0].is_cuda
    clean_seen, attacked_seen = metric.seen[:2], metric.seen[2:]
    assert all(v is None for b in clean_seen for v in b)
    assert all(v is not None and v > 0 for b in attacked_seen for v in b) and len(attacked_seen) == 2
    names = ne.NuScenesDetectionScore().class_names
    keys = {f"NuScenes/{c}_AP_dist_{t}" for c in names for t in ("0.5", "1.0", "2.0", "4.0")}
    keys |= {f"NuScenes/{c}_{e}_err" for c in names for e in ne.TP_METRICS}
    keys |= {"NuScenes/" + k for k in ("mAP", "mATE", "mASE", "mAOE", "mAVE", "mAAE", "NDS")}
    nan_keys = {f"NuScenes/traffic_cone_{e}_err" for e in ("attr", "vel", "orient")} | \
        {f"NuScenes/barrier_{e}_err" for e in ("attr", "vel")}
    assert set(rep) == {"clean", "attacked", "drop"}
    for part in ("clean", "attacked"):
        assert set(rep[part]) == keys
        for k, v in rep[part].items():
            assert isinstance(v, float) and (math.isnan(v) if k in nan_keys else math.isfinite(v)), (part, k, v)
        assert 0.0 <= rep[part]["NuScenes/mAP"] <= 1.0 and 0.0 <= rep[part]["NuScenes/NDS"] <= 1.0
    assert all(_close(rep["drop"][k], rep["clean"][k] - rep["attacked"][k], 0.0) for k in keys)
    second = evaluate(model, batches, ne.NuScenesDetectionScore(), attacked=False)
    assert all(_close(second[k], rep["clean"][k], 0.0) for k in keys)
    print("detections per frame", metric._nd, "clean mAP", rep["clean"]["NuScenes/mAP"], "NDS", rep["clean"]["NuScenes/NDS"])
