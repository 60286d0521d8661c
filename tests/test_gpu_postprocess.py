"""Detection post-processing on the device (csrc/postprocess.hip through robustpointclouds_amd/postprocess.py,
Anchor3DHead / CenterHead `predict_by_feat`, the detectors' `predict`) against the float64 oracle
tests/_postprocess_ref.py."""
import functools

import numpy as np
import pytest
import torch

from tests import _postprocess_cases as cs
from tests import _postprocess_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------- IoU pairs
@functools.lru_cache(maxsize=None)
def _iou_case():
    a, b = cs.random_pairs(4096, seed=0)
    da, db, want = cs.degenerate_pairs()
    a, b = np.concatenate([a, da]), np.concatenate([b, db])
    f64 = np.array([ref.bev_iou(x, y) for x, y in zip(a, b)])
    f32 = np.array([float(ref.bev_iou(x, y, np.float32)) for x, y in zip(a, b)])
    return a, b, f64, f32, want


def test_bev_iou_pairs():
    """4096 random pairs (about half overlapping) + the degenerate table. Tolerance: the oracle's algorithm
    run in numpy float32 differs from float64 by at most 1.37e-5 over these pairs (the 1e-3 m sliver against a
    large box; 1.6e-7 over the random pairs alone); the kernel's bound is 4 x that = 5.5e-5 (operation order,
    fused multiply-adds). Measured on the MI355X: 1.75e-7."""
    from robustpointclouds_amd import postprocess as pp
    a, b, f64, f32, want = _iou_case()
    assert 0.4 < (f64[:4096] > 0).mean() < 0.6
    ref_err = np.abs(f32 - f64).max()
    bound = 4.0 * ref_err
    got = pp.bev_iou_pairs(_dev(a), _dev(b)).cpu().numpy()
    err = np.abs(got.astype(np.float64) - f64).max()
    print(f"fp32 reference error {ref_err:.3e}, bound {bound:.3e}, kernel error {err:.3e}")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    assert 1e-7 < ref_err < 1e-4            # the reference itself is a sane fp32 yardstick
    assert err <= bound
    tail = got[4096:]
    assert tail[0] == 1.0 and tail[1] == 1.0                       # identical boxes
    for g, w in zip(tail, want):
        if w == 0.0:
            assert g == 0.0                                        # touching / degenerate: exactly 0


def test_bev_iou_pairs_extreme_inputs_stay_finite():
    from robustpointclouds_amd import postprocess as pp
    big = np.float32(3e38)
    a = np.array([[0, 0, big, big, 0], [big, -big, 1, 1, 1e30], [0, 0, 1e-30, 1e-30, 0], [1e20, 1e20, 1e19, 1, 3]],
                 dtype=np.float32)
    b = np.array([[0, 0, big, big, 1], [-big, big, big, 1, -1e30], [0, 0, 1e-30, 1e-30, 0], [1e20, 1e20, 1, 1e19, 2]],
                 dtype=np.float32)
    got = pp.bev_iou_pairs(_dev(a), _dev(b)).cpu().numpy()
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0


# ----------------------------------------------------------------------------------- rotated NMS
@functools.lru_cache(maxsize=None)
def _nms_case(thr):
    boxes, counts, ious, worst = cs.nms_groups(thr, seed=0)
    want = [ref.nms_bev_sorted(boxes[g, :n], thr, iou=ious[g]) for g, n in enumerate(counts)]
    return boxes, counts, want, worst


@pytest.mark.parametrize("thr", [0.01, 0.2, 0.5])
def test_nms_bev_batched(thr):
    """G = 8 groups of 0 .. 1000 boxes (word and tile boundaries) in one call; keep sets equal the oracle's."""
    from robustpointclouds_amd import postprocess as pp
    boxes, counts, want, worst = _nms_case(thr)
    assert counts == cs.NMS_COUNTS and worst <= 0.02   # boxes dropped as too close to thr: at most 2 % of a group
    keep, nkeep = pp.nms_bev_batched(_dev(boxes), torch.tensor(counts, device=DEV), thr)
    keep, nkeep = keep.cpu(), nkeep.cpu()
    assert nkeep.tolist() == [len(w) for w in want]
    for g, w in enumerate(want):
        assert keep[g, :len(w)].tolist() == w
        assert (keep[g, len(w):] == -1).all()
    # max_keep below the survivor count: the scan stops there
    cap = 17
    assert sum(len(w) > cap for w in want) >= 4
    keep, nkeep = pp.nms_bev_batched(_dev(boxes), torch.tensor(counts, device=DEV), thr, max_keep=cap)
    assert tuple(keep.shape) == (len(counts), cap)
    assert nkeep.cpu().tolist() == [min(len(w), cap) for w in want]
    for g, w in enumerate(want):
        assert keep[g, :min(len(w), cap)].cpu().tolist() == w[:cap]


def test_nms_bev_at_the_cap():
    """A group of RPC_NMS_MAX_N = 4096 boxes: all 64 words of `removed`, lane 63 included."""
    from robustpointclouds_amd import _ffi
    from robustpointclouds_amd import postprocess as pp
    thr = 0.2
    boxes, counts, ious, worst = cs.nms_groups(thr, seed=1, counts=[_ffi.NMS_MAX_N, 65])
    assert boxes.shape[1] == 4096 and worst <= 0.02
    keep, nkeep = pp.nms_bev_batched(_dev(boxes), torch.tensor(counts, device=DEV), thr)
    keep, nkeep = keep.cpu(), nkeep.cpu()
    for g, n in enumerate(counts):
        w = ref.nms_bev_sorted(boxes[g, :n], thr, iou=ious[g])
        assert int(nkeep[g]) == len(w) and keep[g, :len(w)].tolist() == w
        assert len(w) > n // 3 and w[-1] >= n - 64


def test_nms_entry_argument_errors():
    """max_n above the cap and malformed arguments return non-zero before any launch (null device pointers
    would fault otherwise)."""
    from robustpointclouds_amd import _ffi
    lib = _ffi.load()
    st = _ffi.stream_of(torch.zeros(1, device=DEV))
    assert _ffi.NMS_MAX_N >= 4096
    n = _ffi.NMS_MAX_N + 1
    assert lib.rpc_nms_workspace_size(1, n) == 0
    assert lib.rpc_nms_bev(None, None, 1, n, 0.5, 4, None, None, None, 0, st) == 3
    assert lib.rpc_nms_circle(None, None, None, 1, n, 4, None, None, None, 0, st) == 3
    assert lib.rpc_nms_bev(None, None, 1, 64, 0.5, 4, None, None, None, 0, st) == 1
    assert lib.rpc_nms_bev(None, None, -1, 64, 0.5, 4, None, None, None, 0, st) == 1
    assert lib.rpc_bev_iou_pairs(None, None, 5, None, st) == 1
    x = torch.zeros((1, 64, 5), device=DEV)
    c = torch.zeros(1, dtype=torch.int32, device=DEV)
    k = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    assert lib.rpc_nms_bev(_ffi.ptr(x), _ffi.ptr(c), 1, 64, 0.5, 4, _ffi.ptr(k), _ffi.ptr(c), None, 0, st) == 2
    with pytest.raises(RuntimeError, match="rpc_nms_bev"):
        from robustpointclouds_amd import postprocess as pp
        pp.nms_bev_batched(torch.zeros((1, n, 5), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), 0.5)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------- circle NMS
@pytest.mark.parametrize("case", [0, 1])
def test_nms_circle_batched(case):
    """G = 6 groups with the nuScenes min_radius list as radii; centres on an exact grid, with pairs at
    squared distance exactly equal to the radius (<= must suppress them)."""
    from robustpointclouds_amd import postprocess as pp
    xy, counts = cs.circle_groups(cs.CIRCLE_COUNTS[case])
    rad = cs.NUS_MIN_RADIUS
    exact = 0
    for g, n in enumerate(counts):
        p = xy[g, :n].astype(np.float64)
        d = ((p[:, None] - p[None]) ** 2).sum(-1)
        exact += int(np.triu(d == rad[g], 1).sum())
    assert exact >= 10
    keep, nkeep = pp.nms_circle_batched(_dev(xy), torch.tensor(counts, device=DEV),
                                        torch.tensor(rad, dtype=torch.float32, device=DEV))
    keep, nkeep = keep.cpu(), nkeep.cpu()
    for g, n in enumerate(counts):
        w = ref.circle_nms_sorted(xy[g, :n], rad[g])
        assert int(nkeep[g]) == len(w) and keep[g, :len(w)].tolist() == w
        assert 0 < len(w) < n or n <= 2
    keep, nkeep = pp.nms_circle_batched(_dev(xy), torch.tensor(counts, device=DEV),
                                        torch.tensor(rad, dtype=torch.float32, device=DEV), max_keep=9)
    for g, n in enumerate(counts):
        w = ref.circle_nms_sorted(xy[g, :n], rad[g], max_keep=9)
        assert int(nkeep[g]) == len(w) and keep[g, :len(w)].cpu().tolist() == w


# ----------------------------------------------------------------------------------- Anchor3DHead
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_anchor_predict_by_feat(layout):
    """B = 2, H = W = 8, the KITTI 3-class head with the config's own test_cfg (nms_pre 100, max_num 50):
    frame 0 exceeds max_num with candidates under two labels, frame 1 has no detection."""
    head = cs.kitti_head()
    cfg = cs.kitti_cfg()["test_cfg"]
    assert head.test_cfg == cfg and cfg["max_num"] == 50 and cfg["nms_pre"] == 100
    cls, reg, dcl = cs.head_maps(2, 8, 8, seed=11, bias=(-3.0, -12.0))
    want = cs.anchor_oracle(head, cls, reg, dcl, cfg)
    free = cs.anchor_oracle(head, cls, reg, dcl, dict(cfg, max_num=10 ** 6))
    assert len(free[0][2]) > cfg["max_num"] == len(want[0][2]) and len(want[1][2]) == 0
    assert len(free[0][3]) > len(set(free[0][3].tolist()))            # anchors kept under two labels
    assert min(np.bincount(free[0][2], minlength=3)) >= 3             # several boxes per class
    assert cs.distinct(free[0][1])
    maps = [m.to(DEV) for m in (cls, reg, dcl)]
    if layout == "nhwc":   # the head's own outputs are NCHW views of an NHWC image
        maps = [m.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for m in maps]
    got = head.predict_by_feat([maps[0]], [maps[1]], [maps[2]])
    assert all(g["bboxes_3d"].is_cuda for g in got)
    cs.check_detections(got, want)
    # below max_num: class-major order
    cfg2 = dict(cfg, max_num=10 ** 6)
    cs.check_detections(head.predict_by_feat(maps[0], maps[1], maps[2], cfg2), free)


# ----------------------------------------------------------------------------------- CenterHead
def test_center_predict_by_feat():
    """Packed buffers, B = 2, H = W = 16, tasks [1, 2], max_per_img 40, post_max_size 5, min_radius
    [4, 0.85]: centres west of post_center_limit_range and beyond it in z, scores under the threshold."""
    head = cs.center_head()
    hm, box = cs.center_buffers()
    B, H, W, _ = hm.shape
    cfg, pcr = head.test_cfg, head.train_cfg["point_cloud_range"]
    assert (cfg["max_per_img"], cfg["post_max_size"], cfg["min_radius"]) == (40, 5, [4, 0.85])
    want = ref.center_predict(hm.numpy(), box.numpy(), head.num_classes, cfg, pcr)
    loose = ref.center_predict(hm.numpy(), box.numpy(), head.num_classes,
                               dict(cfg, post_center_limit_range=[-1e9] * 3 + [1e9] * 3, score_threshold=None,
                                    post_max_size=40, min_radius=[-1, -1]), pcr)
    for w, l in zip(want, loose):
        assert cs.distinct(l[1]) and len(l[2]) == 80
        x, z = l[0][:, 0], l[0][:, 2] + l[0][:, 5] * 0.5
        assert (x < -61.2).any() and (np.abs(z) > 10).any() and (l[1] < 0.1).any()
        assert 0 < len(w[2]) <= 10 and {1, 2} & set(w[2].tolist())     # the second task's labels are offset by 1
    preds = ([dict(_packed=(hm.to(DEV).view(B * H * W, -1), box.to(DEV).view(B * H * W, -1), B, H, W))],)
    got = head.predict_by_feat(preds)
    cs.check_detections(got, want)
    cs.check_detections(head.predict_by_feat(preds, dict(cfg, post_max_size=40, score_threshold=None)),
                        ref.center_predict(hm.numpy(), box.numpy(), head.num_classes,
                                           dict(cfg, post_max_size=40, score_threshold=None), pcr))
    # z is the bottom centre: the decoded centre minus half the height
    g, w = got[0], want[0]
    assert np.abs(g["bboxes_3d"][:, 2].double().cpu().numpy() - w[0][:, 2]).max() <= 1e-5
    with pytest.raises(NotImplementedError, match="rotate"):
        head.predict_by_feat(preds, dict(cfg, nms_type="rotate"))


# ----------------------------------------------------------------------------------- detector wiring
def test_voxelnet_predict_is_head_predict_by_feat():
    """AdversarialVoxelNet.predict equals the oracle applied to the maps predict itself fed to the head
    (captured with a forward hook), whatever engine or BatchNorm mode produced them."""
    from robustpointclouds_amd.synthetic import kitti_batch
    from robustpointclouds_amd.trainer import make_kitti_model
    torch.manual_seed(3)
    model = make_kitti_model(num_classes=3, device=DEV, epoch=3)
    head = model.bbox_head
    seen = []
    hook = head.register_forward_hook(lambda m, i, o: seen.append(o))
    pts, _, _ = kitti_batch(2, seed0=21, num_classes=3)
    data = dict(inputs=dict(points=[torch.from_numpy(p[::2]).to(DEV) for p in pts]), data_samples=None)
    # an untrained head scores every anchor at its 0.01 prior, and the empty part of the scene gives many cells
    # the same logits: rescale the class convolution so that each channel's median (the empty cells) sits at
    # logit -8 and the strongest cell at +2, whatever the scale of the features; box deltas within +-0.5 (boxes of a
    # realistic size: the 1e-5 absolute tolerance is for metres, not for exp(3) * anchor),
    # direction logits to std 1
    model.val_step(data)
    cls0, reg0, dir0 = [o[0].float() for o in seen.pop()]
    with torch.no_grad():
        med = cls0.permute(1, 0, 2, 3).reshape(cls0.shape[1], -1).median(1).values
        gain = 10.0 / (cls0 - med[None, :, None, None]).max()
        head.conv_cls.bias.copy_(-8.0 - gain * (med - head.conv_cls.bias))
        head.conv_cls.weight.mul_(gain)
        head.conv_reg.weight.mul_(0.5 / reg0.abs().max())
        head.conv_dir_cls.weight.mul_(1.0 / dir0.std())
    out = model.val_step(data)
    hook.remove()
    assert len(seen) == 1 and len(out) == 2
    cls, reg, dcl = [o[0].detach().float().cpu() for o in seen[0]]
    want = cs.anchor_oracle(head, cls, reg, dcl, head.test_cfg)
    print("detections per frame", [len(w[2]) for w in want])
    assert sum(len(w[2]) for w in want) >= 4
    assert all(cs.distinct(w[1]) for w in want)
    cs.check_detections(out, want)
    assert set(out[0]) >= {"bboxes_3d", "scores_3d", "labels_3d"}
    if model._current_l2_norm is not None:
        assert all(o["perturbation_l2_norm"] == float(model._current_l2_norm) for o in out)
