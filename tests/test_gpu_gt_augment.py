"""GT-database augmentation on the GPU (csrc/gt_augment.hip) against tests/_gt_augment_ref.py.

The cases (tests/_gt_augment_cases.py) keep every decision away from rounding noise, so decisions compare
exactly: first / bitmask / counts, accept, chosen, which points survive and in which order, out_offsets, the
slots boxes land in. Coordinates: a scene point no transform touched is bit-exact; a pasted or noise-moved
point and a moved box centre are within 8 * 2^-17 m (8 ulp at 128 m) of the float64 reference, a yaw within
8 * 2^-22 rad; the NaN tail is all NaN.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import voxelize as ov
from robustpointclouds_amd import GpuObjectNoise, GpuObjectSample, GtDatabase, _ffi, points_in_boxes
from robustpointclouds_amd.pipeline import GpuTrainAugment, concat_frames
from robustpointclouds_amd.synthetic import KITTI_PC_RANGE, KITTI_VOXEL_SIZE
from robustpointclouds_amd.voxelize import voxelize_batch
from tests import _gt_augment_cases as cs
from tests import _gt_augment_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _close_rows(got, want64, tol):
    """xyz within tol of the float64 reference, the other columns bit-equal."""
    assert got.shape == want64.shape, (got.shape, want64.shape)
    if len(got):
        err = np.abs(got[:, :3].astype(np.float64) - want64[:, :3]).max()
        assert err <= tol, err
        assert np.array_equal(_bits(got[:, 3:]), _bits(want64[:, 3:].astype(np.float32)))


# ------------------------------------------------------------------------------------------ points in boxes
@pytest.mark.parametrize("k", range(len(cs.PIB_CASES)))
def test_points_in_boxes_matches_the_reference(k):
    case = cs.pib_case(k)
    pts, off = concat_frames(case["frames"], DEV)
    gb, gl = _dev(case["boxes"]), _dev(case["labels"])
    first, mask, counts = points_in_boxes(pts, off, gb, gl)
    assert np.array_equal(first.cpu().numpy(), case["first"])
    assert np.array_equal(mask.cpu().numpy().view(np.uint32), case["mask"])
    assert np.array_equal(counts.cpu().numpy(), case["counts"])
    if case["M"] > 1:      # the overlapping pair: more memberships than owned points
        assert case["counts"].sum() > (case["first"] >= 0).sum() > 0
    only_first, none, _ = points_in_boxes(pts, off, gb, gl, with_mask=False)
    assert none is None and torch.equal(only_first, first)
    # rows past offsets[B] belong to no frame, wherever they lie
    inside_a_box = case["frames"][2][:3].copy()
    inside_a_box[:, :3] = case["boxes"][2, 0, :3] + np.array([0, 0, 0.5 * case["boxes"][2, 0, 5]], np.float32)
    longer = torch.cat([pts, _dev(inside_a_box)])
    f2, m2, c2 = points_in_boxes(longer, off, gb, gl)
    assert torch.equal(f2[:len(pts)], first) and (f2[len(pts):] == -1).all() and (m2[len(pts):] == 0).all()
    assert torch.equal(c2, counts)


def test_points_in_boxes_caps_and_bad_arguments_launch_nothing():
    lib = _ffi.load()
    P, B, F = 8, 1, 4
    pts = torch.tensor([1.0, 1.0, 1.5, 0.0], device=DEV).repeat(P, 1)      # the centre of the unit box at (1, 1, 1)
    off = torch.tensor([0, P], dtype=torch.int32, device=DEV)

    def call(M, points=pts, n=P, offsets=off):
        gb = torch.ones(B, M, 7, device=DEV)
        gl = torch.zeros(B, M, dtype=torch.long, device=DEV)
        first = torch.full((P,), 77, dtype=torch.int32, device=DEV)
        mask = torch.full((P, (M + 31) // 32), 77, dtype=torch.int32, device=DEV)
        counts = torch.full((B, M), 77, dtype=torch.int32, device=DEV)
        rc = lib.rpc_points_in_boxes(_ffi.ptr(points), F, n, _ffi.ptr(offsets), B, _ffi.ptr(gb), _ffi.ptr(gl), M,
                                     _ffi.ptr(first), _ffi.ptr(mask), _ffi.ptr(counts), _ffi.stream_of(pts))
        torch.cuda.synchronize()
        return rc, first, mask, counts

    rc, first, mask, counts = call(_ffi.GT_MAX_BOXES + 1)
    assert rc == 3 and (first == 77).all() and (mask == 77).all() and (counts == 77).all()
    rc, first, mask, counts = call(_ffi.GT_MAX_BOXES)
    assert rc == 0 and (first == 0).all() and (counts[0] == P).all() and (mask == -1).all()
    for bad in (dict(points=None), dict(n=-1), dict(offsets=None)):
        rc, first, _, counts = call(4, **bad)
        assert rc == 1 and (first == 77).all() and (counts == 77).all()
    with pytest.raises(RuntimeError):
        points_in_boxes(pts, off, torch.ones(B, 129, 7, device=DEV), torch.zeros(B, 129, dtype=torch.long, device=DEV))
    # zero points and zero boxes are no-ops that still write their outputs
    f0, m0, c0 = points_in_boxes(pts[:0], torch.zeros(2, dtype=torch.int32, device=DEV),
                                 torch.ones(B, 3, 7, device=DEV), torch.zeros(B, 3, dtype=torch.long, device=DEV))
    assert f0.numel() == 0 and (c0 == 0).all()
    f1, m1, c1 = points_in_boxes(pts, off, torch.ones(B, 0, 7, device=DEV), torch.zeros(B, 0, dtype=torch.long, device=DEV))
    assert (f1 == -1).all() and m1.shape == (P, 0) and c1.shape == (B, 0)


# ------------------------------------------------------------------------------------------ the database
def test_from_frames_crops_the_reference_objects_and_pastes_them_back():
    case = cs.pib_case(1)
    pts, off = concat_frames(case["frames"], DEV)
    db = GtDatabase.from_frames(pts, off, _dev(case["boxes"]), _dev(case["labels"]), cs.CLASSES)
    want = []
    for b, fr in enumerate(case["frames"]):
        want += [(b, m, p, idx) for m, p, idx in ref.crop_objects(fr, case["boxes"][b], case["labels"][b])]
    assert len(db) == len(want) and len(db) > 10
    shared = 0
    for i, (b, m, p, idx) in enumerate(want):
        assert np.array_equal(db.boxes_host[i], case["boxes"][b, m]) and db.labels_host[i] == case["labels"][b, m]
        assert db.num_points_host[i] == len(idx)
        _close_rows(db.object_points(i).cpu().numpy(), p, cs.COORD_TOL)        # centred, original order
        if i and want[i - 1][0] == b and len(np.intersect1d(want[i - 1][3], idx)):
            shared += 1
    assert shared >= 1                                                          # the overlapping pair shares points
    # round trip: each object of frame 1 pasted at its own box into an empty frame gives its points back
    objs = [i for i, w in enumerate(want) if w[0] == 1]
    B, M = len(objs), 2
    gb = torch.ones(B, M, 7, device=DEV)
    gl = torch.full((B, M), -1, dtype=torch.long, device=DEV)
    cand = np.array(objs, np.int32)[:, None]
    out, out_off, gb, gl, accept = GpuObjectSample(db, cs.GROUPS, cs.CLASSES)(
        pts[:0], torch.zeros(B + 1, dtype=torch.int32, device=DEV), gb, gl, samples=(cand, np.zeros_like(cand)))
    assert (accept == 0).all()
    o = out_off.cpu().numpy()
    assert np.array_equal(o, np.concatenate([[0], np.cumsum(db.num_points_host[objs])]))
    for j, i in enumerate(objs):
        b, m, p, idx = want[i]
        _close_rows(out[o[j]:o[j + 1]].cpu().numpy(), case["frames"][b][idx].astype(np.float64), cs.COORD_TOL)
        assert np.array_equal(gb[j, 0].cpu().numpy(), case["boxes"][b, m]) and int(gl[j, 0]) == case["labels"][b, m]


# ------------------------------------------------------------------------------------------ ObjectSample
@pytest.mark.parametrize("k", [0, 1])
def test_object_sample_matches_the_reference(k):
    case = cs.sample_case(k)
    db = GtDatabase.from_objects(case["objects"], cs.CLASSES, device=DEV)
    pts, off = concat_frames(case["frames"], DEV)
    gb, gl = _dev(case["gt_boxes"]), _dev(case["gt_labels"])
    out, out_off, gb, gl, accept = GpuObjectSample(db, cs.GROUPS, cs.CLASSES)(
        pts, off, gb, gl, samples=(case["cand"], case["draw"]))
    res = case["ref"]
    B = len(res)
    assert np.array_equal(accept.cpu().numpy(), np.stack([r["accept"] for r in res]))
    assert np.array_equal(gl.cpu().numpy(), np.stack([r["labels"] for r in res]))
    assert np.array_equal(_bits(gb.cpu().numpy()), _bits(np.stack([r["boxes"] for r in res])))   # copies of fp32 boxes
    o = out_off.cpu().numpy()
    out = out.cpu().numpy()
    n = 0
    for b in range(B):
        assert o[b] == n
        k_p = len(res[b]["pasted"])
        got = out[o[b]:o[b + 1]]
        assert len(got) == k_p + len(res[b]["kept"])
        _close_rows(got[:k_p], res[b]["pasted"], cs.COORD_TOL)
        assert np.array_equal(_bits(got[k_p:]), _bits(case["frames"][b][res[b]["kept"]]))           # untouched: bit for bit
        n += len(got)
    assert o[B] == n
    cap = len(pts) + sum(len(case["objects"][c][0]) for c in case["cand"].ravel() if c >= 0)
    assert out.shape[0] == cap and cap > n and np.isnan(out[n:]).all()
    assert any(len(r["kept"]) < len(f) for r, f in zip(res, case["frames"]))                        # something was removed


# ------------------------------------------------------------------------------------------ ObjectNoise
@pytest.mark.parametrize("k", range(len(cs.NOISE_CASES)))
def test_object_noise_matches_the_reference(k):
    case = cs.noise_case(k)
    pts, off = concat_frames(case["frames"], DEV)
    gb, gl = _dev(case["gt_boxes"]), _dev(case["gt_labels"])
    out, gb, chosen = GpuObjectNoise(num_try=case["T"])(pts, off, gb, gl, noise=(case["loc"], case["rot"]))
    res = case["ref"]
    assert np.array_equal(chosen.cpu().numpy(), np.stack([r["chosen"] for r in res]))
    o = off.cpu().numpy()
    out, gbh = out.cpu().numpy(), gb.cpu().numpy()
    for b, r in enumerate(res):
        got, src = out[o[b]:o[b + 1]], case["frames"][b]
        assert np.array_equal(_bits(got[~r["moved"]]), _bits(src[~r["moved"]]))                     # unmoved: bit for bit
        _close_rows(got[r["moved"]], r["points"][r["moved"]], cs.COORD_TOL)
        still = r["chosen"] < 0
        assert np.array_equal(_bits(gbh[b][still]), _bits(case["gt_boxes"][b][still]))
        mv = gbh[b][~still].astype(np.float64)
        if len(mv):
            assert np.abs(mv[:, :3] - r["boxes"][~still][:, :3]).max() <= cs.COORD_TOL
            assert np.abs(mv[:, 6] - r["boxes"][~still][:, 6]).max() <= cs.YAW_TOL
            assert np.array_equal(mv[:, 3:6], r["boxes"][~still][:, 3:6])
    if case["special"]:
        assert res[1]["moved"].any() and (res[1]["owner"] == 1).any() and not res[1]["moved"][res[1]["owner"] == 1].any()


def test_nothing_to_do_still_writes_the_outputs():
    case = cs.sample_case(1)
    db = GtDatabase.from_objects(case["objects"], cs.CLASSES, device=DEV)
    pts, off = concat_frames(case["frames"], DEV)
    gb, gl = _dev(case["gt_boxes"]), _dev(case["gt_labels"])
    B = len(case["frames"])
    # no candidate in the whole batch: the scene comes back as it is, with nothing behind it
    none = (np.zeros((B, 0), np.int32), np.zeros((B, 0), np.int32))
    out, out_off, gb2, gl2, accept = GpuObjectSample(db, cs.GROUPS, cs.CLASSES)(pts, off, gb.clone(), gl.clone(),
                                                                                samples=none)
    assert accept.shape == (B, 0) and torch.equal(out_off, off) and torch.equal(gb2, gb) and torch.equal(gl2, gl)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(pts.cpu().numpy()))
    # no tries, and no box slots
    same, gb3, chosen = GpuObjectNoise(num_try=0)(pts.clone(), off, gb.clone(), gl,
                                                  noise=(np.zeros((B, 8, 0, 3), np.float32), np.zeros((B, 8, 0), np.float32)))
    assert (chosen == -1).all() and torch.equal(gb3, gb) and np.array_equal(_bits(same.cpu().numpy()), _bits(pts.cpu().numpy()))
    e_b, e_l = torch.ones(B, 0, 7, device=DEV), torch.zeros(B, 0, dtype=torch.long, device=DEV)
    same, _, chosen = GpuObjectNoise(num_try=4)(pts.clone(), off, e_b, e_l)
    assert chosen.shape == (B, 0) and np.array_equal(_bits(same.cpu().numpy()), _bits(pts.cpu().numpy()))
    # no frames: every row is past the last frame
    first, mask, counts = points_in_boxes(pts, off[:1], gb[:0], gl[:0])
    assert (first == -1).all() and (mask == 0).all() and counts.shape == (0, gl.shape[1])


# ------------------------------------------------------------------------------------------ the chain
def _run_chain(case):
    """ObjectSample -> ObjectNoise -> GpuTrainAugment -> hard_voxelize, nothing read back in between."""
    db = GtDatabase.from_objects(case["objects"], cs.CLASSES, device=DEV)
    pts, off = concat_frames(case["frames"], DEV)
    gb, gl = _dev(case["gt_boxes"]), _dev(case["gt_labels"])
    p1, o1, gb, gl, accept = GpuObjectSample(db, cs.GROUPS, cs.CLASSES)(pts, off, gb, gl,
                                                                        samples=(case["cand"], case["draw"]))
    p2, gb, chosen = GpuObjectNoise(num_try=case["T"])(p1, o1, gb, gl, noise=(case["loc"], case["rot"]))
    p3, o3, gb, gl = GpuTrainAugment(KITTI_PC_RANGE, shuffle=None)(p2, o1, gb, gl, frames=case["aug_frames"])
    vox = voxelize_batch(p3, o3, KITTI_VOXEL_SIZE, KITTI_PC_RANGE, 5, 16000)
    return accept, chosen, p3, o3, gb, gl, vox


@pytest.mark.parametrize("side_stream", [False, True])
def test_chain_sample_noise_augment_voxelize(side_stream):
    case = cs.chain_case()
    if side_stream:      # inputs are uploaded on the side stream too: kernels on any other stream would not see them
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got = _run_chain(case)
        s.synchronize()
    else:
        got = _run_chain(case)
    accept, chosen, p3, o3, gb, gl, (v, c, n, _) = got
    res = case["ref"]
    B = len(res)
    assert np.array_equal(accept.cpu().numpy(), np.stack([r["accept"] for r in res]))
    assert np.array_equal(chosen.cpu().numpy(), np.stack([r["chosen"] for r in res]))
    o = o3.cpu().numpy()
    out = p3.cpu().numpy()
    frames = []
    for b, r in enumerate(res):
        got_b = out[o[b]:o[b + 1]]
        assert len(got_b) == len(r["points"])
        t = r["touched"]
        assert np.array_equal(_bits(got_b[~t]), _bits(r["points"][~t]))
        _close_rows(got_b[t], r["points"][t].astype(np.float64), cs.CHAIN_TOL)
        frames.append(got_b)
        assert np.array_equal(gl[b].cpu().numpy(), r["labels"])
        live = r["labels"] >= 0
        gbh = gb[b].cpu().numpy().astype(np.float64)[live]
        assert np.abs(gbh[:, :6] - r["boxes"][live][:, :6]).max() <= cs.CHAIN_TOL
        assert np.abs(gbh[:, 6] - r["boxes"][live][:, 6]).max() <= cs.CHAIN_YAW_TOL
    assert np.isnan(out[o[B]:]).all() and len(out) > o[B]
    # the NaN tail goes through the voxeliser without a host read of the counts
    rv, rc, rn = ov.voxelize_frames(frames, KITTI_VOXEL_SIZE, KITTI_PC_RANGE, 5, 16000)
    assert np.array_equal(c.cpu().numpy(), rc) and np.array_equal(n.cpu().numpy(), rn)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), rv.view(np.uint32))
