"""CPU: the host side of the KITTI tracklet extraction (alignnet3d/tracklets.py, make_kitti_dataset.py's parser) against the reference's
recorded outputs (tests/golden/tracklet_vectors.*, made by tests/golden/make_tracklet_golden.py), the restatement (tests/tracklet_ref.py)
against scipy's Delaunay -- the reference's method --, and two wrong kernels restated in NumPy that the GPU tests' inputs must refuse."""
import json
import os

import numpy as np
import pytest

from alignnet3d import tracklets as T
from tests import tracklet_cases as C
from tests import tracklet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CHUNK = 1024   # only sizes the random frames here; the GPU tests read the engine's option


def _golden():
    return np.load(os.path.join(GOLD, "tracklet_vectors.npz")), json.load(open(os.path.join(GOLD, "tracklet_vectors.json")))


def _camera(points):
    p = np.asarray(points, np.float64)
    return np.stack([-p[:, 1], -p[:, 2], p[:, 0]], 1)


def test_corners_labels_and_transforms_match_the_reference():
    z, meta = _golden()
    assert len(z["boxes"]) == meta["boxes"] == 40 and np.abs(z["boxes"][:, 6]).max() > np.pi
    for i, (b1, b2) in enumerate(zip(z["boxes1"], z["boxes2"])):
        np.testing.assert_allclose(T.box_corners(b1), z["corners"][i], rtol=0, atol=1e-12)
        mat, tr, ang, cen, zd = T.relative_transform(b1, b2)
        np.testing.assert_allclose(mat, z["rel_transform"][i], rtol=0, atol=1e-12)
        np.testing.assert_allclose(tr, z["translation"][i], rtol=0, atol=1e-12)
        np.testing.assert_allclose(cen, z["rotation_center"][i], rtol=0, atol=1e-12)
        assert abs(ang - z["rel_angle"][i]) <= 1e-12 and abs(zd - z["z_difference"][i]) <= 1e-12
        lab, zd2 = T.labels12(b1, b2)
        want = np.concatenate([z["translation"][i], [z["rel_angle"][i]], z["position1"][i], z["position2"][i], [z["angle1"][i], z["angle2"][i]]])
        np.testing.assert_allclose(lab, want, rtol=0, atol=1e-12)
        assert zd2 == zd and lab[2] == 0.0
    assert np.abs(z["rel_angle"]).max() < np.pi   # (the drawn steps are small; the unwrapped difference is checked below)
    lab, _ = T.labels12([0, 0, 0, 1, 1, 1, 3.0], [0, 0, 0, 1, 1, 1, -3.0])
    assert lab[3] == -6.0   # rel_angle is NOT wrapped: the reference leaves it (pointcloud.py:896)


def test_membership_matches_the_reference_hull_test():
    z, meta = _golden()
    total = 0
    for i in range(meta["hull_boxes"]):
        q = z["hull_points"][i].astype(np.float64)                       # camera frame
        velo = np.stack([q[:, 2], -q[:, 0], -q[:, 1]], 1).astype(np.float32)   # exact: sign changes of float32 values
        decided = ~R.undecided(velo, z["boxes"][i])
        assert np.array_equal(R.inside(velo, z["boxes"][i])[decided], z["hull_inside"][i][decided])
        total += int(z["hull_inside"][i].sum())
    assert total > 100 and total == sum(meta["inside_per_box"])


def test_restatement_agrees_with_delaunay_on_random_rotated_boxes():
    """The reference's method (Delaunay(corners).find_simplex(p) >= 0, pointcloud.py:769-772) on 600 random rotated boxes x 4,000 float32
    points in an 8 m cube around the box, at frame offsets 0, 50 and 5,000 m: no disagreement outside the undecided band, at most 1e-4 of
    the points undecided -- and on these inputs none."""
    from scipy.spatial import Delaunay
    g = np.random.RandomState(0)
    n_pts = n_und = n_dis = 0
    for offset in (0.0, 50.0, 5000.0):
        for _ in range(200):
            box = C.draw_box(g, offset)
            velo = C.points_around(g, box, 4000)
            hull = Delaunay(T.box_corners(box)).find_simplex(_camera(velo)) >= 0
            mine, und = R.inside(velo, box), R.undecided(velo, box)
            n_pts += len(velo); n_und += int(und.sum()); n_dis += int(((mine != hull) & ~und).sum())
            assert 0 < mine.sum() < 2000   # (the smallest drawn box holds 0.1 % of the cube, the largest 3.4 %)
    print("points %d undecided %d disagreements %d" % (n_pts, n_und, n_dis))
    assert n_pts == 2400000 and n_dis == 0
    assert n_und <= 1e-4 * n_pts and n_und == 0


LABEL_TEXT = """\
0 1 Car 0 0 -1.5 10.0 20.0 30.0 40.0 1.5 1.6 3.9 1.0 1.7 20.0 0.1
0 2 Pedestrian 0 1 0.3 10.0 20.0 30.0 40.0 1.7 0.6 0.8 -3.0 1.6 12.0 -2.0
0 -1 DontCare -1 -1 -10 1.0 2.0 3.0 4.0 -1000 -1000 -1000 -10 -1 -1 -1
1 1 Car 1 2 -1.5 10.0 20.0 30.0 40.0 1.5 1.6 3.9 1.2 1.7 20.5 0.15
1 3 Van 0 0 0.0 10.0 20.0 30.0 40.0 2.0 1.9 5.0 6.0 1.8 30.0 1.0

2 1 Car 3 0 -1.5 10.0 20.0 30.0 40.0 1.5 1.6 3.9 1.4 1.7 21.0 0.2
2 2 Pedestrian 0 4 0.3 10.0 20.0 30.0 40.0 1.7 0.6 0.8 -3.1 1.6 12.3 -2.1
3 1 Car 0 3 -1.5 10.0 20.0 30.0 40.0 1.5 1.6 3.9 1.6 1.7 21.5 0.123456789
3 2 Pedestrian 0 0 0.3 10.0 20.0 30.0 40.0 1.7 0.6 0.8 -3.2 1.6 12.6 -2.2
4 2 Pedestrian 0 0 0.3 10.0 20.0 30.0 40.0 1.7 0.6 0.8 -3.3 1.6 12.9 -2.3
5 1 Car 0 0 -1.5 10.0 20.0 30.0 40.0 1.5 1.6 3.9 2.0 1.7 22.5 0.3
"""


def _labels(tmp_path):
    path = tmp_path / "0007.txt"
    path.write_text(LABEL_TEXT)
    return T.read_labels(str(path))


def test_label_parsing_and_filters(tmp_path):
    lab = _labels(tmp_path)
    # dropped: DontCare; frame 2 track 1 (truncated 3 > 2); frame 2 track 2 (occluded 4 > 3).  Kept: occluded 3 and truncated 2 (closed thresholds)
    assert list(zip(lab.frame, lab.track)) == [(0, 1), (0, 2), (1, 1), (1, 3), (3, 1), (3, 2), (4, 2), (5, 1)]
    assert lab.cls[:4] == ["Car", "Pedestrian", "Car", "Van"] and "DontCare" not in lab.cls
    assert lab.box.dtype == np.float64 and lab.box.shape == (8, 7) and lab.bbox2d.shape == (8, 4)
    # (x, y, z, h, w, l, ry) from the file's h w l x y z ry, parsed as float32 and widened (KittiTrackingLabels :621-623)
    f32 = lambda v: float(np.float32(v))
    assert list(lab.box[0]) == [f32(1.0), f32(1.7), f32(20.0), f32(1.5), f32(1.6), f32(3.9), f32(0.1)]
    assert lab.box[4, 6] == f32(0.123456789) != 0.123456789
    assert lab.occluded[2] == 2 and lab.truncated[2] == 1 and lab.occluded[4] == 3
    with pytest.raises(ValueError):
        bad = tmp_path / "bad.txt"
        bad.write_text("0 1 Car 0 0 1 2 3\n")
        T.read_labels(str(bad))


def test_pairing_respects_holes_classes_and_gap(tmp_path):
    lab = _labels(tmp_path)
    key = lambda ps: [(p.track, p.frames) for p in ps]
    # track 1: frames 0, 1, (2 filtered), 3, 5; track 2: frames 0, (2 filtered), 3, 4
    assert key(T.pairs(lab, ("Car",), gap=1)) == [(1, (0, 1))]                      # no pair across the hole 1 -> 3
    assert key(T.pairs(lab, ("Car", "Pedestrian"), gap=1)) == [(1, (0, 1)), (2, (3, 4))]
    assert key(T.pairs(lab, ("Car",), gap=2)) == [(1, (1, 3)), (1, (3, 5))]         # gap = 2: exactly two frames apart
    assert key(T.pairs(lab, ("Pedestrian",), gap=3)) == [(2, (0, 3))]
    assert T.pairs(lab, ("Van",), gap=1) == [] and T.pairs(lab, ("Cyclist",)) == []
    p = T.pairs(lab, ("Car",), gap=1, seq=7)[0]
    assert p.seq == 7 and p.cls == "Car" and np.array_equal(p.box1, lab.box[0]) and np.array_equal(p.box2, lab.box[2]) and p.rows == (0, 2)
    counts = np.array([5, 50, 50, 50, 50, 50, 3, 50])
    assert key(T.pairs(lab, ("Car", "Pedestrian"), gap=1, min_points=10, counts=counts)) == []
    assert key(T.pairs(lab, ("Car", "Pedestrian"), gap=1, min_points=3, counts=counts)) == [(1, (0, 1)), (2, (3, 4))]
    with pytest.raises(ValueError):
        T.pairs(lab, ("Car",), gap=0)
    with pytest.raises(ValueError):
        T.pairs(lab, ("Car",), min_points=5)
    kept, idx = T.filter_min_points(["a", "b", "c"], np.array([[0, 0], [4, 9], [4, 12], [10, 20]]), 4)
    assert (kept, idx) == (["a", "c"], [0, 2])


def test_meta_keys_and_their_order(tmp_path):
    lab = _labels(tmp_path)
    p = T.pairs(lab, ("Car",), gap=1, seq=7)[0]
    m = T.meta(p)
    assert list(m) == ["start_position", "start_angle", "end_position", "end_angle", "translation", "rel_angle", "class", "truncated", "occluded",
                       "seq", "frames", "trackids", "vo1", "vo2", "bbox3ds", "bbox2ds"]
    json.loads(json.dumps(m))
    import provider
    l12, zd = T.labels12(p.box1, p.box2)
    assert np.array_equal(provider.str_to_np(m["translation"]), l12[0:3]) and m["rel_angle"] == l12[3]
    assert np.array_equal(provider.str_to_np(m["start_position"]), l12[4:7]) and np.array_equal(provider.str_to_np(m["end_position"]), l12[7:10])
    assert (m["start_angle"], m["end_angle"]) == (p.box1[6], p.box2[6]) and m["frames"] == [0, 1] and m["trackids"] == [1, 1] and m["class"] == "Car"
    assert np.array_equal(provider.str_to_np(m["vo1"]), np.eye(4)) and np.array_equal(provider.str_to_np(m["bbox3ds"][1]), p.box2)
    # start_position: the box's location in the Velodyne frame, raised by h / 2 (get_transform_components); z_difference leaves the translation
    assert np.allclose(l12[4:7], [p.box1[2], -p.box1[0], -p.box1[1] + p.box1[3] / 2]) and zd == -(p.box2[1] - p.box1[1]) and l12[2] == 0
    # a pose file: R4^T vo R4 (pointcloud.py:848-851) -- a camera-frame translation (1, 2, 3) is (3, -1, -2) in the Velodyne frame
    vo = np.eye(4, dtype=np.float32)
    vo[:3, 3] = [1, 2, 3]
    got = provider.str_to_np(T.meta(p, vo1=vo)["vo1"])
    assert np.array_equal(got[:3, 3], [3, -1, -2]) and np.array_equal(got[:3, :3], np.eye(3))


def test_cli_parser():
    import make_kitti_dataset as M
    a = M.parse_args(["--kitti", "/k", "--out", "/o"])
    assert (a.classes, a.gap, a.min_points, a.val_seqs, a.vo_dir, a.device) == (["Car"], 1, 1, [], None, 0)
    a = M.parse_args(["--kitti", "/k", "--out", "/o", "--classes", "Car,Pedestrian", "--gap", "3", "--min-points", "20", "--val-seqs", "19,2", "--vo-dir", "/v"])
    assert (a.classes, a.gap, a.min_points, a.val_seqs, a.vo_dir) == (["Car", "Pedestrian"], 3, 20, [2, 19], "/v")
    for bad in (["--out", "/o"], ["--kitti", "/k", "--out", "/o", "--gap", "0"], ["--kitti", "/k", "--out", "/o", "--val-seqs", "x"],
                ["--kitti", "/k", "--out", "/o", "--classes", ","]):
        with pytest.raises(SystemExit):
            M.parse_args(bad)


def _members(case, fn):
    out = []
    for b in range(len(case["frames"])):
        for k in range(2):
            out.append(fn(case["scans"][case["frames"][b, k]], case["boxes"][b, k]))
    return out


def test_wrong_kernels_pass_the_easy_inputs_and_are_refused_by_the_hard_ones():
    """An all-float32 membership test and an open box (< for <=), restated: both agree with the definition on the random frames, the closed
    faces refuse the open box, and the far frame refuses the float32 test.  The restatement finds no undecided point on any GPU input."""
    easy = C.random_frames(CHUNK, 4)
    assert sum(int(m.sum()) for m in _members(easy, R.inside)) > 200
    for wrong in (R.inside_f32, R.inside_open):
        assert all(np.array_equal(a, b) for a, b in zip(_members(easy, wrong), _members(easy, R.inside)))
    faces = C.closed_faces()
    want = R.inside(faces["scans"][0], faces["boxes"][0, 0])
    assert np.array_equal(want, faces["expected"]) and want.sum() == 27 + 54 and (~want).sum() == 54
    n_open = int((R.inside_open(faces["scans"][0], faces["boxes"][0, 0]) != want).sum())
    assert n_open == 74   # every inside point but the middle and the six face centres stepped inwards sits on a face in some axis
    far = C.far_frame()
    mine, f32 = _members(far, R.inside), _members(far, R.inside_f32)
    wrong = [int((a != b).sum()) for a, b in zip(mine, f32)]
    print("float32 test misclassifies per job:", wrong[::2])
    assert all(w > 0 for w in wrong) and sum(int(m.sum()) for m in mine) > 1000
    assert all(np.array_equal(a, b) for a, b in zip(mine, _members(far, R.inside_open)))        # no point sits exactly on a face there
    for case in (easy, C.random_frames(CHUNK, 3), faces, far):
        und = sum(int(m.sum()) for m in _members(case, R.undecided))
        assert und == (2 * 74 if case is faces else 0)   # the closed faces' boundary points have gap 0 by construction (both clouds of the pair): exact, not uncertain
