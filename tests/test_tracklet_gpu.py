"""GPU: the KITTI tracklet extraction (include/alignnet_hip.h alignnet_tracklet_*, csrc/alignnet_crop.hip) through the C ABI against the
fp64 restatement tests/tracklet_ref.py.  Bars: the offsets are equal, every point the restatement decides (|gap| >= 1e-9, the project's bar
elsewhere; at most 1e-3 of the points may be undecided, and tests/test_tracklet_cpu.py asserts that these inputs have none but the exact
boundary points of the closed-face case) is in or out as the restatement says, and the crops are the scan's points bit for bit, in scan
order.  Inputs: tests/tracklet_cases.py."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from alignnet3d import scenes as S
from alignnet3d import tracklets as T
from tests import tracklet_cases as C
from tests import tracklet_ref as R
from tests.helpers import small_cfg, oracle_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
SEED = 11


@pytest.fixture(scope="module")
def eng(gpu_required):
    cfg = small_cfg(N=64, nb=12)
    _, P32 = oracle_params(cfg)
    e = alignnet3d.Engine(cfg)
    e.set_variables(P32)
    yield e
    e.close()


def _run(eng, case):
    eng.tracklet_upload_scans(case["scans"])
    off = eng.tracklet_extract(case["frames"], case["boxes"], case["dz"])
    return (off,) + eng.tracklet_read(off)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(eng, case, name, exact=False):
    """One extraction against the restatement.  exact: no point may be undecided but those with gap == 0 (decided by exact arithmetic), and the
    result is the restatement's bit for bit; otherwise undecided points may differ, up to 1e-3 of the points.  Returns the device result."""
    off, p1, p2 = _run(eng, case)
    roff, r1, r2 = R.extract(case["scans"], case["frames"], case["boxes"], case["dz"])
    n_pts = n_und = 0
    for b in range(len(case["frames"])):
        for k in range(2):
            g = R.gap(case["scans"][case["frames"][b, k]], case["boxes"][b, k])
            n_pts += len(g)
            with np.errstate(invalid="ignore"):
                n_und += int(((np.abs(g) < R.UNDECIDED) & (g != 0 if exact else True)).sum())
    print("%s: %d pairs, %d point tests, %d undecided, crops of %d + %d points" % (name, len(case["frames"]), n_pts, n_und, len(p1), len(p2)))
    assert n_und <= 1e-3 * n_pts and n_und == 0   # with none undecided, "equal where decided" is plain equality
    assert off.dtype == np.int64 and np.array_equal(off, roff)
    assert np.array_equal(_bits(p1), _bits(r1)) and np.array_equal(_bits(p2), _bits(r2))
    return off, p1, p2


# ---- 1. random frames ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 4])
def test_random_frames_against_the_restatement(eng, stride):
    chunk = eng.get_option("tracklet_chunk")
    case = C.random_frames(chunk, stride)
    assert sorted(len(s) for s in case["scans"]) == [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1] and case["scans"][-1].shape[1] == stride
    off, p1, p2 = _check(eng, case, "random frames, stride %d" % stride)
    assert len(p1) > 100 and len(p2) > 100 and (np.diff(off[:, 0]) > 0).sum() >= 8
    # the members are points of the scan in scan order: every crop is the scan filtered by a mask
    for b in (len(case["frames"]) - 1, len(case["frames"]) - 3):
        scan = case["scans"][case["frames"][b, 0]]
        assert np.array_equal(_bits(p1[off[b, 0]:off[b + 1, 0]]), _bits(scan[R.inside(scan, case["boxes"][b, 0]), :3]))


# ---- 2. closed faces ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 4])
def test_closed_faces_exactly(eng, stride):
    case = C.closed_faces(stride)
    off, p1, _ = _check(eng, case, "closed faces", exact=True)
    assert off[1, 0] == case["expected"].sum() == 81
    assert np.array_equal(_bits(p1), _bits(case["scans"][0][case["expected"], :3]))


# ---- 3. the decision is fp64 --------------------------------------------------------------------------------------------------------------------------
def test_far_frame_is_decided_in_fp64(eng):
    case = C.far_frame()
    assert np.abs(case["scans"][0][:, :2]).max() > 4000 and {0.0} < set(np.round(case["boxes"][:, 0, 6], 6))
    off, p1, p2 = _check(eng, case, "far frame")
    assert np.array_equal(off[:, 0], off[:, 1]) and np.array_equal(_bits(p1), _bits(p2)) and np.diff(off[:, 0]).min() > 100
    # what an all-float32 test would have returned differs for every job (tests/test_tracklet_cpu.py asserts the same on the CPU)
    for b in range(len(case["frames"])):
        assert not np.array_equal(R.inside_f32(case["scans"][0], case["boxes"][b, 0]), R.inside(case["scans"][0], case["boxes"][b, 0]))


# ---- 4. job-list edges --------------------------------------------------------------------------------------------------------------------------------
def _edge_case(eng):
    g = np.random.RandomState(2)
    per_pass = eng.get_option("tracklet_jobs_per_pass")
    box = np.array([3.0, 1.5, 20.0, 1.6, 1.8, 4.2, 0.7])
    scan = C.points_around(g, box, 700, half=3.0)
    scan[5] = [np.nan, 1.0, 1.0]; scan[70] = [20.0, np.inf, -1.0]; scan[300] = [20.0, -3.0, -np.inf]; scan[699] = [np.nan, np.nan, np.nan]
    scan[6] = [20.0, -3.0, -0.7]   # a point well inside `box`, next to the NaN
    other = C.points_around(g, box, 90, half=3.0)           # a frame no job uses
    third = C.points_around(g, box + [0.5, 0, 0.5, 0, 0, 0, 0], 130, half=1.0)
    everything = np.array([3.0, 10.0, 20.0, 20.0, 20.0, 20.0, 0.3])               # takes every (finite) point of `scan`
    nothing = np.array([300.0, 1.5, 20.0, 1.6, 1.8, 4.2, 0.0])                    # no hit
    zero = np.array([3.0, 0.7, 20.0, 0.0, 0.0, 0.0, 0.0])                         # zero extent
    zero_hit = np.array([-float(scan[6, 1]), -float(scan[6, 2]), float(scan[6, 0]), 0.0, 0.0, 0.0, 0.0])   # zero extent ON a scan point: closed, so it holds it
    wide = box.copy(); wide[6] = 0.7 + 2 * np.pi                                   # |ry| > pi: the same box
    neg = box.copy(); neg[6] = 0.7 - 4 * np.pi
    overlap = box + [0.8, 0.1, 0.6, 0, 0, 0, 0.2]
    boxes = [[box, box], [box, overlap], [everything, nothing], [zero, zero_hit], [wide, neg], [overlap, everything]]
    frames = [[0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 2]]
    while 2 * len(boxes) < per_pass + 1:   # more jobs on frame 0 than one LDS pass stages
        b = C.draw_box(g); b[:3] = box[:3] + g.uniform(-1.5, 1.5, 3)
        boxes.append([b, box + [0, 0, 0, 0, 0, 0, g.uniform(-3, 3)]]); frames.append([0, 0])
    k = 0
    while sum(f.count(0) for f in frames) < 2 * per_pass + 1:   # ... and more than the 64 whose counts the scatter reads at once: the first pairs again
        boxes.append(boxes[k]); frames.append(frames[k]); k += 1
    dz = np.zeros((len(boxes), 2), np.float32); dz[:, 1] = g.uniform(-0.3, 0.3, len(boxes))
    return dict(scans=[C.pad_stride(scan, 4, g), C.pad_stride(other, 4, g), C.pad_stride(third, 4, g)], frames=np.array(frames, np.int32),
                boxes=np.array(boxes), dz=dz)


def test_job_list_edges(eng):
    case = _edge_case(eng)
    assert 2 * len(case["frames"]) >= eng.get_option("tracklet_jobs_per_pass") + 1 and (case["frames"] == 0).sum() >= 2 * eng.get_option("tracklet_jobs_per_pass") + 1
    off, p1, p2 = _check(eng, case, "job-list edges", exact=True)   # the zero-extent box ON a point: gap == 0, decided by exact arithmetic
    n = np.diff(off, axis=0)
    assert n.reshape(-1)[np.flatnonzero(case["frames"].reshape(-1) == 0)[64:]].all()   # frame 0's jobs past the 64th (they are in job order) are not empty
    scan = case["scans"][0]
    assert n[0, 0] == n[0, 1] > 20                                   # the same box twice
    assert np.array_equal(_bits(p1[off[0, 0]:off[1, 0]]), _bits(p1[off[1, 0]:off[2, 0]]))
    both = R.inside(scan, case["boxes"][1, 0]) & R.inside(scan, case["boxes"][1, 1])
    assert both.sum() > 5                                            # overlapping boxes: a point in two crops
    assert n[2, 0] == 700 - 4 and n[2, 1] == 0                       # every finite point; no hit
    assert n[3, 0] == 0 and n[3, 1] == 1                             # zero extent: nothing, and exactly the point it sits on
    assert n[4, 0] == n[4, 1] == n[0, 0]                             # |ry| > pi
    assert np.isfinite(p1).all() and np.isfinite(p2).all()           # NaN / inf coordinates are in no crop
    empty = eng.tracklet_extract(np.zeros((0, 2), np.int32), np.zeros((0, 2, 7)))   # B = 0
    assert empty.shape == (1, 2) and not empty.any() and all(len(p) == 0 for p in eng.tracklet_read(empty))


# ---- 5. batch independence ----------------------------------------------------------------------------------------------------------------------------
def test_batch_independence_and_order(eng):
    case = C.random_frames(eng.get_option("tracklet_chunk"), 4)
    off, p1, p2 = _run(eng, case)
    B = len(case["frames"])
    for b in range(B):
        o, q1, q2 = (eng.tracklet_extract(case["frames"][b:b + 1], case["boxes"][b:b + 1], case["dz"][b:b + 1]),) + eng.tracklet_read()
        assert np.array_equal(o[1], off[b + 1] - off[b])
        assert np.array_equal(_bits(q1), _bits(p1[off[b, 0]:off[b + 1, 0]])) and np.array_equal(_bits(q2), _bits(p2[off[b, 1]:off[b + 1, 1]]))
    perm = np.random.RandomState(1).permutation(B)
    o, q1, q2 = (eng.tracklet_extract(case["frames"][perm], case["boxes"][perm], case["dz"][perm]),) + eng.tracklet_read()
    for i, b in enumerate(perm):
        assert np.array_equal(_bits(q1[o[i, 0]:o[i + 1, 0]]), _bits(p1[off[b, 0]:off[b + 1, 0]]))
        assert np.array_equal(_bits(q2[o[i, 1]:o[i + 1, 1]]), _bits(p2[off[b, 1]:off[b + 1, 1]]))


# ---- 6. dz --------------------------------------------------------------------------------------------------------------------------------------------
def test_dz_is_one_float32_subtraction(eng):
    case = C.random_frames(eng.get_option("tracklet_chunk"), 4)
    zero = dict(case, dz=np.zeros_like(case["dz"]))
    off0, a1, a2 = _run(eng, zero)
    dz = case["dz"].copy()
    dz[:, 1] = np.float64(0.123456789012345) * np.arange(1, len(dz) + 1)   # the host rounds z_difference to float32 ONCE
    off, b1, b2 = _run(eng, dict(case, dz=dz))
    assert np.array_equal(off, off0) and np.array_equal(_bits(a1), _bits(b1))           # cloud 1 untouched
    assert np.array_equal(_bits(a2[:, :2]), _bits(b2[:, :2]))                           # x, y untouched
    per_point = np.repeat(dz[:, 1].astype(np.float32), np.diff(off[:, 1]))
    assert np.array_equal(_bits(b2[:, 2]), _bits(a2[:, 2] - per_point)) and (a2[:, 2] - per_point).dtype == np.float32
    assert not np.array_equal(b2[:, 2], (a2[:, 2].astype(np.float64) - dz[:, 1].astype(np.float64).repeat(np.diff(off[:, 1]))))   # not an fp64 subtraction


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_result_and_scans_as_they_were(eng):
    case = C.random_frames(eng.get_option("tracklet_chunk"), 4)
    off, p1, p2 = _run(eng, case)
    fr, bx = case["frames"][:2].copy(), case["boxes"][:2].copy()

    def bad(f=None, b=None):
        f2, b2 = fr.copy(), bx.copy()
        if f is not None:
            f2[1, 1] = f
        if b is not None:
            b2[1, 0, b[0]] = b[1]
        return lambda: eng.tracklet_extract(f2, b2)

    calls = [bad(f=len(case["scans"])), bad(f=-1), bad(b=(0, np.nan)), bad(b=(6, np.inf)), bad(b=(3, -0.1)), bad(b=(5, -1e-300)),
             lambda: eng.tracklet_upload_scans([np.zeros((10, 5), np.float32)]), lambda: eng.tracklet_upload_scans([np.zeros((10, 2), np.float32)])]
    for call in calls:
        with pytest.raises(alignnet3d.engine.EngineError):
            call()
        q1, q2 = eng.tracklet_read(off)
        assert np.array_equal(_bits(q1), _bits(p1)) and np.array_equal(_bits(q2), _bits(p2))
    # the scans are still the uploaded ones: the same extraction gives the same result
    o, q1, q2 = (eng.tracklet_extract(case["frames"], case["boxes"], case["dz"]),) + eng.tracklet_read()
    assert np.array_equal(o, off) and np.array_equal(_bits(q1), _bits(p1)) and np.array_equal(_bits(q2), _bits(p2))
    eng.tracklet_free_scans()
    with pytest.raises(alignnet3d.engine.EngineError):
        eng.tracklet_extract(fr, bx)
    q1, q2 = eng.tracklet_read(off)
    assert np.array_equal(_bits(q1), _bits(p1))


# ---- 8. resident dataset ------------------------------------------------------------------------------------------------------------------------------
def test_installed_crops_are_the_resident_dataset(eng):
    case = C.random_frames(eng.get_option("tracklet_chunk"), 4)
    off, p1, p2 = _run(eng, case)
    lab = np.stack([T.labels12(b[0], b[1])[0] for b in case["boxes"]]).astype(np.float32)
    eng.tracklet_install_dataset(lab)
    rows = [len(lab) - 1, 0, 3, len(lab) - 2, 8]
    dev = eng.forward_rows(rows, SEED)
    reg = eng.register_rows(rows, SEED, refine="point", radius=1.0)
    # extracting again does not disturb the installed copy
    eng.tracklet_extract(case["frames"][:1], case["boxes"][:1])
    assert all(np.array_equal(dev[k], v) for k, v in eng.forward_rows(rows, SEED).items())
    eng.upload_dataset(p1, p2, off, lab)
    host = eng.forward_rows(rows, SEED)
    assert set(dev) == set(host) and all(np.array_equal(dev[k], host[k]) for k in host)
    srcs, dsts = [p1[off[r, 0]:off[r + 1, 0]] for r in rows], [p2[off[r, 1]:off[r + 1, 1]] for r in rows]
    ref = eng.register(srcs, dsts, seed=SEED, streams=rows, refine="point", radius=1.0)
    for k in ("transforms", "network_transforms", "fitness", "rmse", "iterations"):   # tests/test_register_gpu.py::test_host_clouds: equal, bit for bit
        np.testing.assert_array_equal(reg[k], ref[k], err_msg=k)


# ---- 9. against the scene generator -------------------------------------------------------------------------------------------------------------------
def _car_box(v, scale, pose, inflate=0.01, negate=False):
    """The oriented bounding box of the posed mesh (world vertex = Rz(angle) (scale v) + position, Velodyne frame) as a KITTI box: the length
    axis is the body's x axis, direction (cos a, sin a, 0) = (-sin a, 0, cos a) in the camera frame = (cos ry, 0, -sin ry): ry = -a - pi / 2."""
    lo, hi = (scale * v).min(0), (scale * v).max(0)
    x, y, z, a = pose
    mid = (lo + hi) / 2
    cx, cy = np.cos(a) * mid[0] - np.sin(a) * mid[1] + x, np.sin(a) * mid[0] + np.cos(a) * mid[1] + y
    ry = -a - np.pi / 2
    return np.array([-cy, -(z + lo[2]) + inflate, cx, hi[2] - lo[2] + 2 * inflate, hi[1] - lo[1] + 2 * inflate, hi[0] - lo[0] + 2 * inflate, -ry if negate else ry])


def test_crops_of_a_generated_scene_are_the_cars_returns(eng):
    mesh = S.load_mesh("builtin", "car", 1)
    eng.scene_upload_meshes([mesh])
    poses = np.array([[[9.0, 1.0, -1.6, 0.4], [-2.0, 11.0, -1.7, -1.2]], [[-8.0, -7.0, -1.5, 2.3], [15.0, 15.0, -1.6, 0.0]]])
    off = eng.scene_generate([0, 0], [6.0, 6.0], poses, sigma=0.0)
    c1, c2 = eng.scene_read(off)
    cars = [c1[off[0, 0]:off[1, 0]], c2[off[0, 1]:off[1, 1]], c1[off[1, 0]:off[2, 0]]]
    car_poses = [poses[0, 0], poses[0, 1], poses[1, 0]]
    assert all(len(c) > 200 for c in cars)
    boxes = [_car_box(mesh[0], 6.0, p) for p in car_poses]
    g = np.random.RandomState(4)
    clutter = np.stack([g.uniform(-25, 25, 4000), g.uniform(-25, 25, 4000), g.uniform(-2.5, 1.5, 4000)], 1).astype(np.float32)
    far = np.ones(len(clutter), bool)
    for b in boxes:
        with np.errstate(invalid="ignore"):
            far &= R.gap(clutter, b) < -0.05
    clutter = clutter[far][:500]
    assert len(clutter) == 500
    frame = C.pad_stride(np.concatenate(cars + [clutter]), 4, g)
    eng.tracklet_upload_scans([frame])
    o = eng.tracklet_extract(np.zeros((3, 2), np.int32), np.array([[b, b] for b in boxes]))
    p1, p2 = eng.tracklet_read(o)
    for i, car in enumerate(cars):
        assert np.array_equal(_bits(p1[o[i, 0]:o[i + 1, 0]]), _bits(car)), "car %d: %d points, crop %d" % (i, len(car), o[i + 1, 0] - o[i, 0])
    assert np.array_equal(_bits(p1), _bits(p2))
    # the designed fail-without case: the yaw negated loses points of the elongated body
    wrong = np.array([[_car_box(mesh[0], 6.0, p, negate=True)] * 2 for p in car_poses])
    ow = eng.tracklet_extract(np.zeros((3, 2), np.int32), wrong)
    lost = [len(car) - int(ow[i + 1, 0] - ow[i, 0]) for i, car in enumerate(cars)]
    print("points per car %s, lost with ry negated %s" % ([len(c) for c in cars], lost))
    assert all(l > 0.05 * len(c) for l, c in zip(lost, cars))


# ---- 10. the command ----------------------------------------------------------------------------------------------------------------------------------
def test_make_kitti_dataset_end_to_end(gpu_required, tmp_path):
    """The command in a fresh process turns a tiny KITTI-shaped tree (2 sequences x 4 frames) into a dataset; its files equal the restatement's
    and provider loads it."""
    kitti, root = tmp_path / "kitti", tmp_path / "KittiTiny"
    C.write_kitti_tree(str(kitti))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    r = subprocess.run([sys.executable, os.path.join(PKG, "make_kitti_dataset.py"), "--kitti", str(kitti), "--out", str(root), "--classes", "Car,Pedestrian",
                        "--min-points", "5", "--val-seqs", "1"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    want = []
    for seq in (0, 1):
        labels = T.read_labels(str(kitti / "training" / "label_02" / ("%04d.txt" % seq)))
        for p in T.pairs(labels, ("Car", "Pedestrian"), gap=1, seq=seq):
            scans = [T.read_scan(str(kitti), seq, f) for f in p.frames]
            assert all(len(s) <= 3000 for s in scans)
            l12, zd = T.labels12(p.box1, p.box2)
            c1, c2 = R.crop(scans[0], p.box1), R.crop(scans[1], p.box2, np.float32(zd))
            if min(len(c1), len(c2)) >= 5:
                want.append((p, c1, c2, l12))
    n_val = sum(1 for w in want if w[0].seq == 1)
    assert len(want) >= 8 and 0 < n_val < len(want) and {w[0].cls for w in want} == {"Car", "Pedestrian"}
    assert "wrote %d pairs (%d train, %d val)" % (len(want), len(want) - n_val, n_val) in r.stdout
    assert [int(x) for x in open(root / "split" / "val.txt").read().split()] == list(range(len(want) - n_val, len(want)))
    assert len(os.listdir(root / "meta")) == len(want)
    for i, (p, c1, c2, l12) in enumerate(want):
        stem = "%08d" % i
        assert json.load(open(root / "meta" / (stem + ".json"))) == json.loads(json.dumps(T.meta(p)))
        for k, c in ((1, c1), (2, c2)):
            pc = np.load(root / ("pointcloud%d" % k) / (stem + ".npy"))
            assert pc.dtype == np.float64 and np.array_equal(pc, c.astype(np.float64)), (i, k)
        assert np.array_equal(np.load(root / "transform" / (stem + ".npy")), T.relative_transform(p.box1, p.box2)[0])
    for m in ("config", "provider"):
        sys.modules.pop(m, None)
    config = importlib.import_module("config")
    try:
        cfgp = tmp_path / "cfg.json"
        json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")}, "model": {"num_points": 16}}, open(cfgp, "w"))
        cfg = config.load_config(str(cfgp))
        assert (cfg.data.ntrain, cfg.data.nval) == (len(want) - n_val, n_val)
        provider = importlib.import_module("provider")
        np.random.seed(0)
        batch = provider.load_batch([0, len(want) - 1], override_batch_size=2)
        assert batch[0].shape == (2, 16, 3)
        for row, i in enumerate((0, len(want) - 1)):
            l12 = want[i][3]
            got = np.concatenate([np.ravel(batch[2][row]), np.ravel(batch[3][row]), np.ravel(batch[4][row]), np.ravel(batch[5][row]), np.ravel(batch[6][row]),
                                  np.ravel(batch[7][row])])
            assert np.array_equal(got, l12)
            assert all((want[i][1].astype(np.float64) == p).all(1).any() for p in batch[0][row][:8])
    finally:
        config.reset_config()
