"""The calibration side of the KITTI evaluator on the device (csrc/kitti_eval.hip: rpc_kitti_project,
rpc_kitti_overlaps_2d, rpc_kitti_match_counts_aos, through robustpointclouds_amd/kitti_eval.py) against the float64
restatement tests/_kitti_calib_ref.py, on the cases of tests/_kitti_calib_cases.py (whose margins
tests/test_kitti_calib_cpu.py checks on the CPU)."""
import numpy as np
import pytest
import torch

from tests import _kitti_calib_cases as cc
from tests import _kitti_calib_ref as cref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FOUR = ("BEV", "3D", "2D", "AOS")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------- projection
def test_project():
    """F = 5 frames of 0, 1, 255, 257, 513 boxes, a matrix and an image size of its own for each, 3 rows past the
    last offset; boxes across the camera plane (corners of negative W), outside the image and the range, a NaN box.
    `valid` is exact. Raw and clipped boxes and the height are held to float64 within 4 x the float32 numpy
    restatement's own maximum error on these boxes; the angle, which the kernel forms in float64, to 1e-12.
    Measured on the MI355X: raw 0.136 px against a bound of 0.707 px (the restatement's own 0.177 px is a corner near
    W = 0.05 m; the kernel rounds every operation in the restatement's order and differs by its sin / cos only),
    clipped 2.36e-4 against 1.29e-3 px, height 6.2e-5 against 3.7e-4 px."""
    from robustpointclouds_amd import kitti_eval as ke
    pc = cc.project_case()
    n = pc["off"][-1]
    assert np.diff(pc["off"]).tolist() == [0, 1, 255, 257, 513] and len(pc["boxes"]) == n + 3
    out = ke.project_boxes(_dev(pc["boxes"]), pc["off"], _dev(pc["mats"]), _dev(pc["hws"]))
    got = {k: v.cpu().numpy() for k, v in out.items()}
    want = {k: np.array([p[k] for p in pc["p64"]], dtype=np.float64) for k in ("raw", "clip", "alpha", "height")}
    valid = np.array([p["valid"] for p in pc["p64"]])
    assert np.array_equal(got["valid"][:n], valid) and 0.3 < valid.mean() < 0.9
    fin = np.isfinite(want["raw"]).all(1)
    assert (~fin).sum() == 2 and np.isnan(got["raw"][:n][~fin]).all() and (got["clip"][:n][~fin] == 0).all()
    for key in ("raw", "clip", "height"):
        ref_err = np.abs(pc["p32"][key][fin].astype(np.float64) - want[key][fin]).max()
        err = np.abs(got[key][:n][fin].astype(np.float64) - want[key][fin]).max()
        print(f"{key}: fp32 reference error {ref_err:.3e}, bound {4 * ref_err:.3e}, kernel error {err:.3e}")
        assert 0 < ref_err and err <= 4.0 * ref_err
    assert np.abs(pc["p32"]["raw"][fin].astype(np.float64) - want["raw"][fin]).max() < 2.0    # a sane yardstick
    afin = np.isfinite(want["alpha"])
    assert got["alpha"].dtype == np.float64 and np.array_equal(np.isfinite(got["alpha"][:n]), afin)
    assert np.abs(got["alpha"][:n][afin] - want["alpha"][afin]).max() < 1e-12
    # rows past the last offset belong to no frame: zeros
    for key in ("raw", "clip", "height", "alpha", "valid"):
        assert not got[key][n:].any()


def test_project_filter_is_exact_and_writes_inside_its_outputs():
    """The detection filter is the flag path (DESIGN.md proves flag -1 equal to absence): the survivors, in order,
    are exactly the reference's valid rows, the per-frame counts of survivors are exact, and the entry writes
    nothing outside [0, n) of any output (sentinel rows on both sides)."""
    from robustpointclouds_amd import _ffi
    pc = cc.project_case()
    n, pad = len(pc["boxes"]), 5
    off = torch.tensor(pc["off"], dtype=torch.int32, device=DEV)
    boxes, mats, hws = _dev(pc["boxes"]), _dev(pc["mats"]), _dev(pc["hws"])
    raw, clip = (torch.full((n + 2 * pad, 4), -7.0, device=DEV) for _ in range(2))
    height = torch.full((n + 2 * pad,), -7.0, device=DEV)
    alpha = torch.full((n + 2 * pad,), -7.0, device=DEV, dtype=torch.float64)
    valid = torch.full((n + 2 * pad,), 9, device=DEV, dtype=torch.uint8)
    p = _ffi.ptr
    rc = _ffi.load().rpc_kitti_project(p(boxes), n, p(off), 5, 513, p(mats), p(hws), _ffi.float_arr(cc.RANGE),
                                       p(raw[pad:]), p(clip[pad:]), p(valid[pad:]), p(alpha[pad:]), p(height[pad:]), None)
    torch.cuda.synchronize()
    assert rc == 0
    for t, s in ((raw, -7.0), (clip, -7.0), (height, -7.0), (alpha, -7.0), (valid, 9)):
        assert (t[:pad] == s).all() and (t[-pad:] == s).all()
    v = valid[pad:pad + pc["off"][-1]].cpu().numpy().astype(bool)
    want = np.array([q["valid"] for q in pc["p64"]])
    assert np.array_equal(np.flatnonzero(v), np.flatnonzero(want))                  # survivors and their order
    counts = [int(v[a:b].sum()) for a, b in zip(pc["off"], pc["off"][1:])]
    assert counts == [int(want[a:b].sum()) for a, b in zip(pc["off"], pc["off"][1:])]   # the new offsets


# ----------------------------------------------------------------------------------- 2D overlaps
def test_overlaps_2d():
    """(Nd, Ng) = (0, 7), (9, 0), (1, 1), (65, 33), (512, 128) and the degenerate table (slivers, shared edges, zero
    area, negative sides). The bound is 4 x the float32 restatement's own maximum error against float64. Measured
    on the MI355X: 1.685e-7 against a bound of 6.74e-7 (the restatement's own error, to the digit)."""
    from robustpointclouds_amd import kitti_eval as ke
    c = cc.overlap2d_case()
    ov, ov_off = ke.box_overlaps_2d(_dev(c["dets"]), c["det_off"], _dev(c["gts"]), c["gt_off"])
    got = ov.cpu().numpy()
    assert got.shape == c["f64"].shape and ov_off[5] == c["n5"] == 1 + 65 * 33 + 512 * 128
    assert 0.2 < (c["f64"][:c["n5"]] > 0).mean() < 0.8
    ref_err = np.abs(c["f32"].astype(np.float64) - c["f64"]).max()
    err = np.abs(got.astype(np.float64) - c["f64"]).max()
    print(f"2D IoU: fp32 reference error {ref_err:.3e}, bound {4 * ref_err:.3e}, kernel error {err:.3e}")
    assert 1e-8 < ref_err < 1e-5 and err <= 4.0 * ref_err
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    for g, w in zip(got[c["n5"]:], c["wants"]):
        if w is not None:
            assert g == w


def test_dontcare_bits():
    """DontCare counts 0, 1 and 64 a frame: the stuff bits of both strict values equal the float64 reference's
    (ratios within 4 x the float32 restatement's error of a value were removed); 65 give the error code."""
    from robustpointclouds_amd import _ffi
    from robustpointclouds_amd import kitti_eval as ke
    c = cc.dc_case()
    assert np.diff(c["dc_off"]).tolist() == [0, 1, 64]
    bits = ke.box_overlaps_2d(_dev(c["dets"]), c["det_off"], _dev(c["dcs"]), c["dc_off"], mode=1,
                              min_overlaps=list(cc.STRICT_VALUES))
    assert bits.dtype == torch.uint8 and np.array_equal(bits.cpu().numpy().astype(bool), c["want"])
    assert c["want"][:, :c["det_off"][1]].sum() == 0 and c["want"].sum() > 10
    with pytest.raises(ValueError):
        ke.box_overlaps_2d(torch.zeros(1, 4, device=DEV), [0, 1], torch.zeros(65, 4, device=DEV), [0, 65], mode=1,
                           min_overlaps=[0.5])
    z = torch.zeros(65 * 4, device=DEV)
    off = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = torch.full((4,), 9, dtype=torch.uint8, device=DEV)
    p = _ffi.ptr
    rc = _ffi.load().rpc_kitti_overlaps_2d(p(z), p(off), p(z), p(off), None, 1, 1, 65, 1, None, p(z), 1, 1, p(out), None)
    torch.cuda.synchronize()
    assert rc == 3 and (out == 9).all()          # RPC_ERR_UNSUPPORTED, nothing written


# ----------------------------------------------------------------------------------- matcher
def _metric(frames, metrics=FOUR):
    from robustpointclouds_amd import kitti_eval as ke
    m = ke.KittiAP(cc.CLASSES, metrics=metrics)
    m.update(*cc.to_update(frames, DEV))
    return m


def _detail(m):
    detail = {}
    counts, nthr = m._counts(detail=detail)
    return counts, nthr, detail


def test_match_counts_aos_on_the_devices_own_overlaps_and_angles():
    """The reference loops fed the DEVICE's fp32 2D overlaps, stuff bits and float64 angles: every tp / fp / fn at
    every threshold is equal, and the similarity sums agree with float64 sums of the same angles within
    n_tp 2^-40: a term is rounded to a multiple of 2^-40 (at most 2^-41 off) and its float64 cosine is off by a few
    1e-16. Twice: bit-identical. With stuff and the angles null the entry equals rpc_kitti_match_counts bit for bit."""
    from robustpointclouds_amd import _ffi
    from robustpointclouds_amd import kitti_eval as ke
    frames = cc.eval_frames()[0]
    m = _metric(frames)
    counts, nthr, detail = _detail(m)
    fams, G = detail["families"], 18
    assert fams == ["BEV", "3D", "2D"] and detail["stuff"] is not None and detail["stuff"].is_cuda
    d_off, g_off, o_off = detail["det_off"], detail["gt_off"], detail["ov_off"]
    cal = detail["calib"]
    valid = cal["valid"].cpu().numpy()
    ov = detail["overlaps"][2].cpu().numpy()
    stuff = detail["stuff"].cpu().numpy()
    a_det, a_gt = cal["det_alpha"].cpu().numpy(), cal["gt_alpha"].cpu().numpy()
    prepared, ov2d, alphas, stuffs = cref.prepare(frames), [], [], []
    for f, pr in enumerate(prepared):
        keep = np.flatnonzero(valid[d_off[f]:d_off[f + 1]])
        assert keep.tolist() == pr["det_keep"]                                   # the filter, frame by frame
        nd, ng = d_off[f + 1] - d_off[f], g_off[f + 1] - g_off[f]
        ov2d.append(ov[o_off[f]:o_off[f + 1]].reshape(nd, ng)[keep])
        alphas.append((a_det[d_off[f]:d_off[f + 1]][keep], a_gt[g_off[f]:g_off[f + 1]]))
        stuffs.append(stuff[:, d_off[f]:d_off[f + 1]][:, keep])
    want = cref.evaluate(prepared, cc.CLASSES, ("2D", "AOS"), ov2d=ov2d, alphas=alphas, stuffs=stuffs)
    cc.assert_equal_to_reference(counts, nthr, detail, want, fams)
    sim = detail["sim"].numpy().astype(np.float64) / ke.SIM_ONE
    n_tp_total = 0
    for (mm, c, d, t), w in want.items():
        if mm != "AOS":
            continue
        g = (c * 3 + d) * 2 + t
        for k, (cnt, s) in enumerate(zip(w["counts"], w["sims"])):
            assert abs(sim[g, k] - s) <= max(cnt[0], 1) * 2.0 ** -40, (c, d, t, k, sim[g, k], s)
            n_tp_total += cnt[0]
        assert not sim[g, len(w["counts"]):].any()
    assert n_tp_total > 1000 and stuff.sum() > 0
    counts2, nthr2, detail2 = _detail(m)
    assert nthr2 == nthr and torch.equal(counts2, counts) and torch.equal(detail2["sim"], detail["sim"])
    # stuff and the angles null: rpc_kitti_match_counts, bit for bit
    frame = (d_off, g_off, o_off, max(np.diff(d_off)), max(np.diff(g_off)),
             ke._device_offsets(d_off, g_off, o_off, DEV))
    k2 = fams.index("2D")
    nthr_t = torch.tensor(nthr[k2 * G:(k2 + 1) * G], dtype=torch.int32, device=DEV)
    mo = detail["min_ov"].view(-1, 2)[:, :1].expand(-1, 2).reshape(-1).contiguous()
    args = (detail["overlaps"][2], frame, detail["score"], detail["flag_det"], detail["flag_gt"], mo, detail["thr"][k2],
            nthr_t)
    plain = ke._match_counts(*args)
    ext, sim0 = ke._match_counts(*args, ext=True)
    assert torch.equal(plain, ext) and not sim0.any()
    with_stuff, _ = ke._match_counts(*args, stuff=detail["stuff"], ext=True)
    assert (with_stuff[..., 1] <= plain[..., 1]).all() and (with_stuff[..., 1] < plain[..., 1]).any()
    assert torch.equal(with_stuff[..., 0], plain[..., 0]) and torch.equal(with_stuff[..., 2], plain[..., 2])


def test_end_to_end_against_float64():
    """All four metrics on about 40 calibrated frames, the frame at the caps (512 detections, 128 ground truths, 64
    DontCare boxes) among them, against the all-float64 reference: counts equal, every AP and AOS within 1e-9
    (measured on the MI355X: 3.4e-12)."""
    frames, share = cc.eval_frames()
    assert share <= cc.MAX_SHARE and 36 <= len(frames) <= 45
    m = _metric(frames)
    counts, nthr, detail = _detail(m)
    want = cref.evaluate(cref.prepare(frames), cc.CLASSES)
    cc.assert_equal_to_reference(counts, nthr, detail, want, detail["families"])
    got, exp = m.compute(), cref.result_dict(want, cc.CLASSES)
    assert set(got) == set(exp) and len(got) == 4 * (3 * 2 * 3 * 2 + 2 * 3)
    worst = max(abs(got[k] - exp[k]) for k in exp)
    print(f"largest |AP - reference| {worst:.3e}")
    assert worst <= 1e-9
    assert 1.0 < got["KITTI/Car_2D_AP40_moderate_strict"] < 100.0
    assert 0.0 < got["KITTI/Car_AOS_AP40_moderate_strict"] < got["KITTI/Car_2D_AP40_moderate_strict"]
    assert got["KITTI/Car_BEV_AP40_easy_strict"] != got["KITTI/Car_BEV_AP40_moderate_strict"]


# ----------------------------------------------------------------------------------- argument errors
def test_argument_errors_return_before_any_launch():
    from robustpointclouds_amd import _ffi
    lib = _ffi.load()
    assert _ffi.KITTI_MAX_DC == 64
    p = _ffi.ptr
    z = torch.zeros(64, device=DEV)
    zd = torch.zeros(64, device=DEV, dtype=torch.float64)
    u8 = torch.full((64,), 9, dtype=torch.uint8, device=DEV)
    off = torch.zeros(2, dtype=torch.int32, device=DEV)
    off64 = torch.zeros(2, dtype=torch.int64, device=DEV)
    rng = _ffi.float_arr(cc.RANGE)
    proj = lambda boxes, n, o, F, mx, mat, hw, r, raw, clip, v, al, h: lib.rpc_kitti_project(
        boxes, n, o, F, mx, mat, hw, r, raw, clip, v, al, h, None)
    good = (p(z), 1, p(off), 1, 1, p(z), p(z), rng, p(z), p(z), p(u8), p(zd), p(z))
    assert proj(*good) == 0                                              # one row of no frame: zeros
    torch.cuda.synchronize()
    assert u8[0] == 0 and (u8[1:] == 9).all()
    for k in (0, 2, 5, 6, 7, 8, 9, 10, 11, 12):                          # every pointer null in turn
        bad = list(good)
        bad[k] = None
        assert proj(*bad) == 1, k
    assert proj(p(z), -1, p(off), 1, 1, p(z), p(z), rng, p(z), p(z), p(u8), p(zd), p(z)) == 1
    assert proj(p(z), 1, p(off), -1, 1, p(z), p(z), rng, p(z), p(z), p(u8), p(zd), p(z)) == 1
    assert proj(p(z), 1, p(off), 1, -1, p(z), p(z), rng, p(z), p(z), p(u8), p(zd), p(z)) == 1
    assert proj(None, 0, None, 0, 0, None, None, rng, None, None, None, None, None) == 0     # nothing to do
    ov2 = lambda *a: lib.rpc_kitti_overlaps_2d(*a, None)
    tail = (None, 0, 0, None)
    assert ov2(p(z), p(off), p(z), p(off), p(off64), 1, 1, 1, 0, p(z), *tail) == 0
    assert ov2(p(z), p(off), p(z), p(off), p(off64), 1, 513, 1, 0, p(z), *tail) == 3
    assert ov2(p(z), p(off), p(z), p(off), p(off64), 1, 1, 129, 0, p(z), *tail) == 3
    assert ov2(p(z), p(off), p(z), p(off), p(off64), -1, 1, 1, 0, p(z), *tail) == 1
    assert ov2(p(z), p(off), p(z), p(off), p(off64), 1, 1, 1, 2, p(z), *tail) == 1
    assert ov2(None, p(off), p(z), p(off), p(off64), 1, 1, 1, 0, p(z), *tail) == 1
    assert ov2(p(z), p(off), p(z), p(off), None, 1, 1, 1, 0, p(z), *tail) == 1
    assert ov2(p(z), p(off), p(z), p(off), p(off64), 1, 1, 1, 0, None, *tail) == 1
    assert ov2(p(z), p(off), p(z), p(off), None, 1, 1, 1, 1, None, p(z), 1, 1, p(u8[8:])) == 0
    assert ov2(p(z), p(off), p(z), p(off), None, 1, 1, 1, 1, None, None, 1, 1, p(u8[8:])) == 1
    assert ov2(p(z), p(off), p(z), p(off), None, 1, 1, 1, 1, None, p(z), 1, 1, None) == 1
    assert ov2(p(z), p(off), p(z), p(off), None, 1, 1, 1, 1, None, p(z), -1, 1, p(u8[8:])) == 1
    assert ov2(p(z), None, p(z), p(off), None, 1, 1, 1, 1, None, p(z), 1, 1, p(u8[8:])) == 1
    torch.cuda.synchronize()
    assert u8[8] == 0 and (u8[9:] == 9).all()                            # only the good call wrote, one element
    flags = torch.zeros(64, dtype=torch.int8, device=DEV)
    cnt = torch.full((41 * 3,), 9, dtype=torch.int32, device=DEV)
    sim = torch.full((41,), 9, dtype=torch.int64, device=DEV)
    nthr = torch.zeros(1, dtype=torch.int32, device=DEV)
    head = (p(z), p(off64), p(off), p(off))
    mid = (p(z), p(flags), p(flags), 1, 1, p(z), 1, 1, p(z), p(nthr))
    aos = lambda *a: lib.rpc_kitti_match_counts_aos(*a, None)
    assert aos(*head, 1, 513, 1, *mid, None, 1, None, None, p(cnt), p(sim)) == 3
    assert aos(*head, 1, 1, 129, *mid, None, 1, None, None, p(cnt), p(sim)) == 3
    assert aos(*head, -1, 1, 1, *mid, None, 1, None, None, p(cnt), p(sim)) == 1
    assert aos(*head, 1, 1, 1, *mid, None, 1, None, None, None, p(sim)) == 1
    assert aos(*head, 1, 1, 1, *mid, None, 1, None, None, p(cnt), None) == 1
    assert aos(*head, 1, 1, 1, *mid, p(u8), 0, None, None, p(cnt), p(sim)) == 1      # no groups per stuff row
    assert aos(*head, 1, 1, 1, p(z), p(flags), p(flags), 1, 1, p(z), 1, 1, None, p(nthr), None, 1, None, None, p(cnt),
               p(sim)) == 1
    torch.cuda.synchronize()
    assert (cnt == 9).all() and (sim == 9).all()
    assert aos(*head, 1, 1, 1, *mid, None, 1, None, None, p(cnt), p(sim)) == 0
    torch.cuda.synchronize()
    assert not cnt.any() and not sim.any()


# ----------------------------------------------------------------------------------- robustness_report
def test_robustness_report_with_four_metrics():
    """The smallest synthetic AdversarialVoxelNet with a synthetic KITTI-like calibration (fx = fy = 721.5, a 375 x
    1242 image, the usual axis permutation): complete keys of all four metrics, values in [0, 100]."""
    from robustpointclouds_amd import kitti_eval as ke
    from robustpointclouds_amd import robustness_report
    from robustpointclouds_amd.synthetic import kitti_batch
    from tests.test_gpu_predict_eval import _data, _model
    model = _model()
    pts, boxes, labels = kitti_batch(2, seed0=21, num_classes=3)
    frames = [p[::4] for p in pts]
    l2i = ke.lidar2img(*cc.calibration(0))
    gts = [dict(bboxes_3d=torch.from_numpy(np.asarray(b, dtype=np.float32)).reshape(-1, 7),
                labels_3d=torch.from_numpy(np.asarray(l, dtype=np.int64)).reshape(-1), lidar2img=l2i,
                img_shape=cc.IMG_HW, dontcare=np.array([[0, 0, 200, 100]], dtype=np.float32))
           for b, l in zip(boxes, labels)]
    batches = [(_data(frames[:1]), gts[:1]), (_data(frames[1:]), gts[1:])]
    rep = robustness_report(model, batches, None, metric=ke.KittiAP(cc.CLASSES, metrics=FOUR))
    torch.cuda.synchronize()
    keys = {f"KITTI/{c}_{m}_AP{r}_{d}_{t}" for c in cc.CLASSES for m in FOUR for r in (11, 40)
            for d in ("easy", "moderate", "hard") for t in ("strict", "loose")}
    keys |= {f"KITTI/Overall_{m}_AP{r}_{d}" for m in FOUR for r in (11, 40) for d in ("easy", "moderate", "hard")}
    assert set(rep) == {"clean", "attacked", "drop"}
    for part in ("clean", "attacked"):
        assert set(rep[part]) == keys
        assert all(isinstance(v, float) and 0.0 <= v <= 100.0 for v in rep[part].values())
        for k in keys:
            if "_AOS_" in k:
                assert rep[part][k] <= rep[part][k.replace("_AOS_", "_2D_")] + 1e-9
    assert all(rep["drop"][k] == rep["clean"][k] - rep["attacked"][k] for k in keys)
