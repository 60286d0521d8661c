"""GT-database augmentation, CPU side: the reference (tests/_gt_augment_ref.py) on hand-checked cases, the
sampler's host logic (need, cursor wrap, seeding, prepare), and the margins every GPU case is built to keep
(tests/_gt_augment_cases.py): no point within 1e-4 m of a face it is tested against, no evaluated box pair
within 1e-3 m of touching."""
import numpy as np
import pytest
import torch

from robustpointclouds_amd import GpuObjectNoise, GpuObjectSample, GtDatabase, points_in_boxes
from tests import _gt_augment_cases as cs
from tests import _gt_augment_ref as ref


def box(x, y, z=0.0, dx=4.0, dy=2.0, dz=1.5, yaw=0.0):
    return np.array([x, y, z, dx, dy, dz, yaw], np.float64)


# ------------------------------------------------------------------------------------------ the reference
def test_point_on_a_z_face_is_inside_and_on_an_x_face_is_outside():
    b = box(0.0, 0.0)
    pts = np.array([[0.0, 0.0, 1.5], [0.0, 0.0, 0.0], [2.0, 0.0, 0.5], [0.0, 1.0, 0.5], [1.999, 0.999, 0.75],
                    [0.0, 0.0, 1.5001], [np.nan, 0.0, 0.5]])
    assert ref.inside(pts, b).tolist() == [True, True, False, False, True, False, False]
    m = ref.inside_margin(pts[:5], b)
    assert m[0] == 0.0 and m[2] == 0.0 and m[4] == pytest.approx(-0.001)
    rot = box(0.0, 0.0, yaw=np.pi / 2)                       # now 2 wide in x and 4 long in y
    assert ref.inside(np.array([[0.0, 1.9, 0.5], [1.1, 0.0, 0.5]]), rot).tolist() == [True, False]
    assert not ref.exists(box(0, 0, dx=0.0), 0) and not ref.exists(b, -1) and ref.exists(b, 2)


def test_rectangles_sharing_an_edge_do_not_collide():
    a, b = box(0.0, 0.0), box(4.0, 0.0)
    assert ref.sep(a, b) == pytest.approx(0.0, abs=1e-12) and not ref.collide(a, b)
    assert ref.collide(a, box(3.99, 0.0)) and ref.sep(a, box(5.0, 0.0)) == pytest.approx(1.0)


def test_rotated_rectangle_inside_the_hull_of_another_does_not_collide():
    a = box(0.0, 0.0, dx=6.0, dy=1.0, yaw=np.pi / 4)         # hull: |x|, |y| <= 2.47
    b = box(1.9, -1.9, dx=1.0, dy=1.0)                       # inside the hull's corner, off the diagonal strip
    hull = 0.5 * (6.0 + 1.0) / np.sqrt(2.0)
    assert abs(b[0]) - 0.5 < hull and abs(b[1]) - 0.5 < hull
    assert ref.sep(a, b) > 0.1 and not ref.collide(a, b) and ref.sep(a, b) == pytest.approx(ref.sep(b, a))
    assert ref.collide(a, box(1.0, 1.0, dx=1.0, dy=1.0))


def test_rule_c_rejects_a_candidate_for_a_later_one_that_is_itself_rejected():
    db = [box(20.0, 0.0), box(40.0, 20.0), box(23.0, 1.0)]   # 0 and 2 overlap; 1 is free
    gt = np.stack([box(26.0, 2.0), box(0, 0, dx=1, dy=1, dz=1)])   # overlaps 2 only; then a free slot
    gl = np.array([0, -1])
    cand, draw = np.array([0, 1, 2]), np.array([0, 0, 0])
    assert not ref.collide(db[0], gt[0]) and ref.collide(db[2], gt[0]) and ref.collide(db[0], db[2])
    acc, boxes, labels = ref.sample_select(cand, draw, db, [0, 0, 0], gt, gl)
    assert acc.tolist() == [-1, 1, -1] and labels.tolist() == [0, 0] and np.array_equal(boxes[1], db[1])
    # in different draws candidate 0 is not held back by candidate 2
    acc, _, _ = ref.sample_select(cand, np.array([0, 0, 1]), db, [0, 0, 0], np.concatenate([gt, gt[1:]]),
                                  np.array([0, -1, -1]))
    assert acc.tolist() == [1, 2, -1]
    # no slot left: rejected, nothing written
    acc, boxes, labels = ref.sample_select(cand, draw, db, [0, 0, 0], gt[:1], gl[:1])
    assert acc.tolist() == [-1, -1, -1] and np.array_equal(boxes, gt[:1])


def test_noise_try_is_tested_against_the_moved_pose_of_an_earlier_box():
    boxes = np.stack([box(20.0, 0.0, dy=1.6), box(20.0, 3.0, dy=1.6), box(50.0, 20.0)])
    labels = np.array([0, 0, 1])
    loc, rot = np.zeros((3, 2, 3)), np.zeros((3, 2))
    loc[0, 0] = (0.0, -1.5, 0.1)
    loc[1, 0] = (0.0, -6.0, 0.0)                             # y = -3: 3.0 from the original box 0, 1.5 from the moved
    loc[1, 1] = (0.3, 0.5, 0.0)
    chosen = ref.noise_select(boxes, labels, loc, rot)
    assert chosen.tolist() == [0, 1, 0]
    still = loc.copy()
    still[0, :] = 0.0
    still[0, :, 0] = 100.0                                   # box 0 goes far away instead: box 1's first try is free
    assert ref.noise_select(boxes, labels, still, rot).tolist()[1] == 0
    pts = np.array([[20.0, 0.0, 0.5, 0.7], [20.0, 3.0, 0.5, 0.1], [0.0, 0.0, 0.0, 0.2]])
    out, nb, owner, moved = ref.noise_apply(pts, boxes, labels, loc, rot, chosen)
    assert owner.tolist() == [0, 1, -1] and moved.tolist() == [True, True, False]
    np.testing.assert_allclose(out[0], [20.0, -1.5, 0.6, 0.7])
    np.testing.assert_allclose(out[1], [20.3, 3.5, 0.5, 0.1])
    np.testing.assert_allclose(nb[1], [20.3, 3.5, 0.0, 4.0, 1.6, 1.5, 0.0])
    # counter-clockwise: a point on the box's +x axis goes to +y under a positive rotation
    rot[2, 0] = np.pi / 2
    out, nb, _, _ = ref.noise_apply(np.array([[51.0, 20.0, 0.5, 0.0]]), boxes, labels, loc, rot, np.array([-1, -1, 0]))
    np.testing.assert_allclose(out[0, :3], [50.0, 21.0, 0.5], atol=1e-12)
    assert nb[2, 6] == pytest.approx(np.pi / 2)


def test_first_box_owns_a_shared_point_and_the_mask_keeps_both():
    boxes = np.stack([box(0.0, 0.0), box(1.0, 0.0), box(1.0, 0.0)])
    first, contains, counts = ref.points_in_boxes_frame(np.array([[0.9, 0.0, 0.5], [2.5, 0.0, 0.5]]), boxes,
                                                        np.array([0, 1, -1]))
    assert first.tolist() == [0, 1] and contains.tolist() == [[True, True, False], [False, True, False]]
    assert counts.tolist() == [1, 2, 0] and ref.pack_mask(contains).tolist() == [[3], [2]]


# ------------------------------------------------------------------------------------------ the sampler's host side
def _db(n_per_class=(7, 5, 3)):
    rng = np.random.default_rng(0)
    objs = []
    for c, n in enumerate(n_per_class):
        for k in range(n):
            b = np.array([10.0 * k, 10.0 * c, 0, 1, 1, 1, 0], np.float32)
            objs.append((cs.object_points(rng, b, 3 + k), b, c, k % 3 - 1))
    return GtDatabase.from_objects(objs, cs.CLASSES, device="cpu")


def test_need_follows_rate_and_the_frame_s_own_labels():
    s = GpuObjectSample(_db(), dict(Car=15, Pedestrian=10, Cyclist=10), cs.CLASSES, rate=0.5)
    labels = np.array([0, 0, 0, 1, 2, 2, -1, -1])
    assert [s.need(c, labels) for c in cs.CLASSES] == [6, 4, 4]    # round(0.5 * 12), round(4.5) = 4 (to even), 4
    full = GpuObjectSample(_db(), dict(Car=3, Pedestrian=0, Cyclist=2), cs.CLASSES)
    assert [full.need(c, labels) for c in cs.CLASSES] == [0, -1, 0]
    cand, draw = full.sample([labels], np.random.RandomState(0))
    assert cand.shape == (1, 0) and draw.shape == (1, 0)


def test_cursor_wrap_returns_a_short_tail_and_reshuffles():
    s = GpuObjectSample(_db(), dict(Car=3, Pedestrian=0, Cyclist=0), cs.CLASSES)
    rng = np.random.RandomState(3)
    empty = np.full(4, -1)
    a, da = s.sample([empty], rng)          # cursor 0 -> 3
    b, _ = s.sample([empty], rng)           # cursor 3 -> 6
    c, _ = s.sample([empty], rng)           # 6 + 3 >= 7: the tail of one, then a new permutation
    d, _ = s.sample([empty], rng)
    assert a.shape == (1, 3) and b.shape == (1, 3) and c.shape == (1, 1) and d.shape == (1, 3)
    assert da.tolist() == [[0, 0, 0]]
    assert sorted(a[0].tolist() + b[0].tolist() + c[0].tolist()) == list(range(7))   # one pass over the 7 cars
    assert len(set(d[0].tolist())) == 3 and s._cursor["Car"] == 3
    # exactly reaching the end also wraps (upstream's >=)
    t = GpuObjectSample(_db((6, 1, 1)), dict(Car=3, Pedestrian=0, Cyclist=0), cs.CLASSES)
    t.sample([empty], rng)
    e, _ = t.sample([empty], rng)
    assert e.shape == (1, 3) and t._cursor["Car"] == 0


def test_same_seed_same_candidates_and_classes_in_order():
    labels = [np.array([0, -1, -1]), np.array([2, 2, 1])]
    runs = [GpuObjectSample(_db(), dict(Car=2, Pedestrian=2, Cyclist=2), cs.CLASSES).sample(
        labels, np.random.RandomState(5)) for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    cand, draw = runs[0]
    assert draw.tolist() == [[0, 1, 1, 2, 2], [0, 0, 1, -1, -1]] and (cand[1, 3:] == -1).all()
    db = _db()
    for b in range(2):
        for c, d in zip(cand[b], draw[b]):
            assert c < 0 or db.labels_host[c] == d
    other = GpuObjectSample(_db(), dict(Car=2, Pedestrian=2, Cyclist=2), cs.CLASSES).sample(
        labels, np.random.RandomState(6))
    assert not np.array_equal(other[0], cand)


def test_prepare_filters_by_difficulty_and_min_points():
    db = _db()
    assert len(db) == 15 and db.num_points_host.tolist()[:7] == [3, 4, 5, 6, 7, 8, 9]
    out = db.prepare(filter_by_difficulty=[-1], filter_by_min_points=dict(Car=5, Pedestrian=4))
    keep = [i for i in range(15) if db.difficulty_host[i] != -1
            and not (db.labels_host[i] == 0 and db.num_points_host[i] < 5)
            and not (db.labels_host[i] == 1 and db.num_points_host[i] < 4)]
    assert 0 < len(keep) < 15 and len(out) == len(keep)
    assert np.array_equal(out.boxes_host, db.boxes_host[keep]) and np.array_equal(out.labels_host, db.labels_host[keep])
    for j, i in enumerate(keep):
        assert torch.equal(out.object_points(j), db.object_points(i))
    assert len(db.prepare(filter_by_difficulty=[], filter_by_min_points=None)) == 15


def test_noise_sample_order_and_unsupported_options():
    n = GpuObjectNoise(num_try=4, translation_std=(1.0, 1.0, 0.5))
    loc, rot = n.sample(2, 3, np.random.RandomState(9))
    rs = np.random.RandomState(9)
    for b in range(2):
        np.testing.assert_array_equal(loc[b], rs.normal(scale=[1.0, 1.0, 0.5], size=[3, 4, 3]).astype(np.float32))
        np.testing.assert_array_equal(rot[b], rs.uniform(-0.78539816, 0.78539816, size=[3, 4]).astype(np.float32))
    with pytest.raises(NotImplementedError):
        GpuObjectNoise(global_rot_range=(0.0, 0.1))


def test_cpu_tensors_raise():
    pts, off = torch.zeros(4, 4), torch.tensor([0, 4], dtype=torch.int32)
    gb, gl = torch.zeros(1, 2, 7), torch.full((1, 2), -1, dtype=torch.long)
    with pytest.raises(RuntimeError):
        points_in_boxes(pts, off, gb, gl)
    with pytest.raises(RuntimeError):
        GpuObjectNoise(num_try=1)(pts, off, gb, gl)
    with pytest.raises(RuntimeError):
        GpuObjectSample(_db(), cs.GROUPS, cs.CLASSES)(pts, off, gb, gl, labels_host=[np.array([-1, -1])])
    with pytest.raises(RuntimeError):
        GtDatabase.from_frames(pts, off, gb, gl, cs.CLASSES)


# ------------------------------------------------------------------------------------------ margins of the GPU cases
def _point_margin(points, boxes):
    m = np.inf
    for b in boxes:
        with np.errstate(invalid="ignore"):
            d = np.abs(ref.inside_margin(points, b))
        if np.isfinite(d).any():
            m = min(m, np.nanmin(d))
    return m


@pytest.mark.parametrize("k", range(len(cs.PIB_CASES)))
def test_pib_cases_keep_the_point_margin(k):
    case = cs.pib_case(k)
    assert [len(f) for f in case["frames"]] == list(cs.PIB_CASES[k]["counts"])
    for b, pts in enumerate(case["frames"]):
        assert _point_margin(pts, case["boxes"][b]) >= cs.PT_MARGIN
    if case["M"] > 1:
        both = np.concatenate([(ref.pack_mask(ref.points_in_boxes_frame(p, case["boxes"][b], case["labels"][b])[1])
                                [:, 0] & 3) == 3 for b, p in enumerate(case["frames"])])
        assert both.any()                                           # first-vs-mask has something to show
        assert (case["labels"][:, 2] == -1).all() and (case["boxes"][:, 4, 3] == 0).all()
        assert np.isnan(np.concatenate(case["frames"])).any()


@pytest.mark.parametrize("k", [0, 1])
def test_sample_cases_keep_both_margins(k):
    case = cs.sample_case(k)
    db_boxes = [o[1] for o in case["objects"]]
    db_labels = [o[2] for o in case["objects"]]
    assert 35 <= len(db_boxes) <= 45 and all(5 <= len(o[0]) <= 200 for o in case["objects"])
    log = []
    for b, pts in enumerate(case["frames"]):
        acc, _, _ = ref.sample_select(case["cand"][b], case["draw"][b], db_boxes, db_labels, case["gt_boxes"][b],
                                      case["gt_labels"][b], log)
        assert np.array_equal(acc, case["ref"][b]["accept"])
        assert _point_margin(pts, [db_boxes[c] for c in case["cand"][b] if c >= 0]) >= cs.PT_MARGIN
    assert len(log) > 20 and min(log) >= cs.SEP_MARGIN
    acc = [r["accept"] for r in case["ref"]]
    if k == 0:
        assert (case["gt_labels"][0] < 0).all() and (case["cand"][2] < 0).all() and 0 not in case["draw"][1]
        assert any((a >= 0).any() for a in acc) and any(((a < 0) & (case["cand"][b] >= 0)).any()
                                                        for b, a in enumerate(acc))
    else:
        assert (acc[0] >= 0).sum() == 2 and sorted(acc[0][acc[0] >= 0].tolist()) == [3, 6]   # the two free slots
        assert acc[1][0] == -1 and acc[1][2] == -1


@pytest.mark.parametrize("k", range(len(cs.NOISE_CASES)))
def test_noise_cases_keep_both_margins(k):
    case = cs.noise_case(k)
    log = []
    for b, pts in enumerate(case["frames"]):
        chosen = ref.noise_select(case["gt_boxes"][b], case["gt_labels"][b], case["loc"][b], case["rot"][b], log)
        assert np.array_equal(chosen, case["ref"][b]["chosen"])
        real = [case["gt_boxes"][b, m] for m in range(case["M"]) if case["gt_labels"][b, m] >= 0]
        assert _point_margin(pts, real) >= cs.PT_MARGIN
    assert not log or min(log) >= cs.SEP_MARGIN
    if case["special"]:
        assert case["ref"][0]["chosen"][:2].tolist() == [0, 1] and case["gt_labels"][0, 2] == -1
        assert case["ref"][1]["chosen"][1] == -1 and case["ref"][1]["chosen"][2] >= 0


def test_chain_case_keeps_its_margins():
    case = cs.chain_case()
    assert any((r["accept"] >= 0).any() for r in case["ref"]) and any((r["chosen"] >= 0).any() for r in case["ref"])
    assert any(r["touched"].any() for r in case["ref"])
