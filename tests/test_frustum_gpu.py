"""GPU: the image-frustum crop (include/alignnet_hip.h alignnet_tracklet_extract_frustum, csrc/alignnet_crop.hip) through the C ABI against
the fp64 restatement tests/frustum_ref.py.  Bars: the offsets are equal, every point the restatement decides (|gap| >= 1e-9; at most 1e-3 of
the points may be undecided, and tests/test_frustum_cpu.py asserts that these inputs have none but the points placed exactly ON an edge) is
in or out as the restatement says, and the crops are the scan's points bit for bit, in scan order.  Inputs: tests/frustum_cases.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from alignnet3d import scenes as S
from alignnet3d import tracklets as T
from tests import frustum_cases as C
from tests import frustum_ref as R
from tests import tracklet_cases as BC
from tests import tracklet_ref as BR
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


def _extract(eng, case, sel=slice(None)):
    off = eng.tracklet_extract_frustum(case["frames"][sel], case["rects"][sel], case["proj"], case["image"], case["dz"][sel], case["clip"])
    return (off,) + eng.tracklet_read(off)


def _run(eng, case):
    eng.tracklet_upload_scans(case["scans"])
    return _extract(eng, case)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


def _check(eng, case, name, exact=False):
    """One extraction against the restatement.  exact: no point may be undecided but those with gap == 0 (decided by exact arithmetic).  With
    none undecided, "equal where decided" is plain equality.  Returns the device result."""
    off, p1, p2 = _run(eng, case)
    roff, r1, r2 = R.extract(case["scans"], case["frames"], case["rects"], case["proj"], case["image"], case["dz"], case["clip"])
    n_pts, n_und = C.undecided_count(case, exact)
    print("%s: %d pairs, %d point tests, %d undecided, crops of %d + %d points" % (name, len(case["frames"]), n_pts, n_und, len(p1), len(p2)))
    assert n_und <= 1e-3 * n_pts and n_und == 0
    assert off.dtype == np.int64 and np.array_equal(off, roff)
    assert np.array_equal(_bits(p1), _bits(r1)) and np.array_equal(_bits(p2), _bits(r2))
    return off, p1, p2


def _crops(case, off, p1, p2):
    """The crops of every job (pair-major, cloud-minor)."""
    return [(p1, p2)[k][off[b, k]:off[b + 1, k]] for b in range(len(case["frames"])) for k in range(2)]


def _masked(case, masks):
    """What the crops must be for the given membership masks (dz = 0)."""
    return [case["scans"][case["frames"][j // 2, j % 2]][m, :3] for j, m in enumerate(masks)]


# ---- 1. random frames ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 4])
def test_random_frames_against_the_restatement(eng, stride):
    chunk = eng.get_option("tracklet_chunk")
    case = C.random_frames(chunk, stride)
    assert sorted(len(s) for s in case["scans"]) == [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1] and case["scans"][-1].shape[1] == stride
    off, p1, p2 = _check(eng, case, "random frames, stride %d" % stride)
    assert len(p1) > 100 and len(p2) > 100 and (np.diff(off[:, 0]) > 0).sum() >= 8


# ---- 2. half-open edges -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 4])
def test_half_open_edges_exactly(eng, stride):
    case = C.half_open_edges(stride)
    off, p1, p2 = _check(eng, case, "half-open edges", exact=True)
    assert off[1, 0] == case["expected"][0].sum() == 6 and off[1, 1] == case["expected"][1].sum() == 19
    assert _same(_crops(case, off, p1, p2), _masked(case, case["expected"]))


# ---- 3. the decision is fp64 --------------------------------------------------------------------------------------------------------------------------
def test_near_edges_are_decided_in_fp64(eng):
    case = C.near_edges()
    off, p1, p2 = _check(eng, case, "near edges")
    crops = _crops(case, off, p1, p2)
    mine, f32 = C.members(case), C.members(case, R.inside_f32)
    for j, (c, keep) in enumerate(zip(case["chosen"], case["kept"])):
        pt = case["scans"][0][c, :3]
        assert mine[j][c] == keep != f32[j][c]          # what an all-float32 projection would have returned differs on every job
        assert (_bits(crops[j]) == _bits(pt)).all(1).any() == keep, j


# ---- 4. clip and behind the camera ----------------------------------------------------------------------------------------------------------------
def test_clip_distance_mirrored_and_non_finite_points(eng):
    case = C.clip_and_behind()
    scan = case["scans"][0]
    assert not np.isfinite(scan[:, :3]).all() and (scan[:, 0] < 0).sum() >= 60 and ((scan[:, 0] > 0) & (scan[:, 0] <= 2)).sum() == 60
    off, p1, p2 = _check(eng, case, "clip and behind", exact=True)
    assert off[1, 0] == off[1, 1] == 70 and _same([p1, p2], _masked(case, [case["expected"]] * 2))
    assert np.isfinite(p1).all() and (p1[:, 0] > 2).all()


# ---- 5. degenerate rectangles -------------------------------------------------------------------------------------------------------------------------
def test_degenerate_rectangles(eng):
    case = C.degenerate_rects()
    off, p1, p2 = _check(eng, case, "degenerate rectangles")
    n = np.diff(off, axis=0)
    W, H = case["image"]
    u, v = R.project(p1, case["proj"])
    assert n[0, 0] > 10 and (u < W).all() and (v < H).all() and (u >= W - 150).all()   # beyond the image: cut at u = W, v = H
    assert n[0, 1] == 0 and n[1, 0] == 0 and n[1, 1] == 0                               # wholly outside, xmin > xmax, zero area: empty, no error


# ---- 6. job-list edges and per-frame calibration --------------------------------------------------------------------------------------------------
def test_job_list_edges_and_per_frame_calibration(eng):
    per_pass = eng.get_option("tracklet_jobs_per_pass")
    case = C.job_list_edges(per_pass)
    assert (case["frames"] == 0).sum() >= 2 * per_pass + 1 and (case["frames"] == 1).sum() >= per_pass + 1 and len(case["scans"][3]) == 0
    assert not np.array_equal(case["proj"][0], case["proj"][1]) and not np.array_equal(case["image"][0], case["image"][1])
    off, p1, p2 = _check(eng, case, "job-list edges")
    n = np.diff(off, axis=0)
    assert (n[:-1] > 0).mean() > 0.8 and not n[-1].any()
    wrong = R.extract(case["scans"], case["frames"], case["rects"], case["proj"], case["image"], case["dz"], frame0_calibration=True)
    assert not np.array_equal(wrong[0], off)                                            # frame 0's calibration for every frame: refused
    empty = eng.tracklet_extract_frustum(np.zeros((0, 2), np.int32), np.zeros((0, 2, 4)), case["proj"], case["image"])   # B = 0
    assert empty.shape == (1, 2) and not empty.any() and all(len(p) == 0 for p in eng.tracklet_read(empty))


# ---- 7. batch independence ----------------------------------------------------------------------------------------------------------------------------
def test_batch_independence_and_order(eng):
    case = C.random_frames(eng.get_option("tracklet_chunk"), 4)
    off, p1, p2 = _run(eng, case)
    B = len(case["frames"])
    for b in range(B):
        o, q1, q2 = _extract(eng, case, slice(b, b + 1))
        assert np.array_equal(o[1], off[b + 1] - off[b])
        assert np.array_equal(_bits(q1), _bits(p1[off[b, 0]:off[b + 1, 0]])) and np.array_equal(_bits(q2), _bits(p2[off[b, 1]:off[b + 1, 1]]))
    perm = np.random.RandomState(1).permutation(B)
    o, q1, q2 = _extract(eng, case, perm)
    for i, b in enumerate(perm):
        assert np.array_equal(_bits(q1[o[i, 0]:o[i + 1, 0]]), _bits(p1[off[b, 0]:off[b + 1, 0]]))
        assert np.array_equal(_bits(q2[o[i, 1]:o[i + 1, 1]]), _bits(p2[off[b, 1]:off[b + 1, 1]]))


# ---- 8. dz --------------------------------------------------------------------------------------------------------------------------------------------
def test_dz_is_one_float32_subtraction(eng):
    case = C.random_frames(eng.get_option("tracklet_chunk"), 4)
    off0, a1, a2 = _run(eng, dict(case, dz=np.zeros_like(case["dz"])))
    dz = case["dz"].copy()
    dz[:, 1] = np.float64(0.123456789012345) * np.arange(1, len(dz) + 1)   # the host rounds z_difference to float32 ONCE
    off, b1, b2 = _run(eng, dict(case, dz=dz))
    assert np.array_equal(off, off0) and np.array_equal(_bits(a1), _bits(b1))           # cloud 1 untouched
    assert np.array_equal(_bits(a2[:, :2]), _bits(b2[:, :2]))                           # x, y untouched
    per_point = np.repeat(dz[:, 1].astype(np.float32), np.diff(off[:, 1]))
    assert np.array_equal(_bits(b2[:, 2]), _bits(a2[:, 2] - per_point)) and (a2[:, 2] - per_point).dtype == np.float32
    assert not np.array_equal(b2[:, 2], (a2[:, 2].astype(np.float64) - dz[:, 1].astype(np.float64).repeat(np.diff(off[:, 1]))))   # not an fp64 subtraction


# ---- 9. errors, and the two extractions side by side --------------------------------------------------------------------------------------------------
def test_errors_leave_result_and_scans_as_they_were(eng):
    case = C.random_frames(eng.get_option("tracklet_chunk"), 4)
    res = _run(eng, case)
    F = len(case["scans"])
    fr, rc, dz = case["frames"][:2].copy(), case["rects"][:2].copy(), case["dz"][:2].copy()
    M, image = np.broadcast_to(case["proj"], (F, 3, 4)).copy(), np.broadcast_to(case["image"], (F, 2)).copy()

    def bad(**kw):
        a = dict(frames=fr.copy(), rects=rc.copy(), proj=M.copy(), image=image.copy(), dz=dz.copy(), clip=2.0)
        for k, (idx, val) in kw.items():
            if idx is None:
                a[k] = val
            else:
                a[k][idx] = val
        return lambda: eng.tracklet_extract_frustum(**a)

    calls = [bad(frames=((1, 1), F)), bad(frames=((0, 0), -1)), bad(rects=((1, 0, 2), np.nan)), bad(rects=((0, 1, 0), -np.inf)), bad(proj=((F - 1, 2, 3), np.nan)),
             bad(proj=((0, 0, 0), np.inf)), bad(image=((3, 0), np.inf)), bad(image=((F - 1, 1), np.nan)), bad(image=((2, 0), 0.0)), bad(image=((0, 1), -375.0)),
             bad(clip=(None, np.nan)), bad(clip=(None, np.inf)), bad(dz=((1, 1), np.nan))]
    lib, h = eng._lib, eng._h
    ip, dp, fp, lp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    args = [fr.ctypes.data_as(ip), rc.ctypes.data_as(dp), dz.ctypes.data_as(fp), 2, M.ctypes.data_as(dp), image.ctypes.data_as(dp), 2.0, lp()]
    for k in (0, 1, 2, 4, 5):   # a null frames, rects, dz, proj, image
        a = list(args)
        a[k] = type(a[k])()
        calls.append(lambda a=a: eng._check(lib.alignnet_tracklet_extract_frustum(h, *a)))
    for call in calls:
        with pytest.raises(alignnet3d.engine.EngineError):
            call()
        assert _same(eng.tracklet_read(res[0]), res[1:])
    # the scans are still the uploaded ones: the same extraction gives the same result
    assert _same(_extract(eng, case), res)
    # a box extraction and a frustum extraction alternate on one engine, each bit-identical to itself alone
    box = BC.random_frames(eng.get_option("tracklet_chunk"), 4)
    eng.tracklet_upload_scans(box["scans"])
    box_res = (eng.tracklet_extract(box["frames"], box["boxes"], box["dz"]),) + eng.tracklet_read()
    assert _same(box_res, BR.extract(box["scans"], box["frames"], box["boxes"], box["dz"]))
    rects = np.array([[C.box_rect(b, case["proj"]) for b in pair] for pair in box["boxes"]])
    both = dict(case, scans=box["scans"], frames=box["frames"], rects=rects, dz=box["dz"])
    fr_res = _extract(eng, both)
    assert _same(fr_res, R.extract(box["scans"], box["frames"], rects, case["proj"], case["image"], box["dz"])) and len(fr_res[1]) > len(box_res[1])
    for _ in range(2):
        assert _same((eng.tracklet_extract(box["frames"], box["boxes"], box["dz"]),) + eng.tracklet_read(), box_res)
        assert _same(_extract(eng, both), fr_res)
    eng.tracklet_free_scans()
    with pytest.raises(alignnet3d.engine.EngineError, match="no scans uploaded"):
        _extract(eng, both)
    assert _same(eng.tracklet_read(fr_res[0]), fr_res[1:])


# ---- 10. resident dataset -----------------------------------------------------------------------------------------------------------------------------
def test_installed_crops_are_the_resident_dataset(eng):
    case = C.random_frames(eng.get_option("tracklet_chunk"), 4)
    off, p1, p2 = _run(eng, case)
    lab = np.random.RandomState(3).uniform(-1, 1, (len(case["frames"]), 12)).astype(np.float32)
    eng.tracklet_install_dataset(lab)
    rows = [r for r in range(len(lab)) if np.diff(off, axis=0)[r].min() > 0][::-3]
    assert len(rows) >= 4
    assert all(eng.sample_batch(rows, SEED)[:2])
    dev = eng.forward_rows(rows, SEED)
    _extract(eng, case, slice(0, 1))   # extracting again does not disturb the installed copy
    assert all(np.array_equal(dev[k], v) for k, v in eng.forward_rows(rows, SEED).items())
    eng.upload_dataset(p1, p2, off, lab)
    host = eng.forward_rows(rows, SEED)
    assert set(dev) == set(host) and all(np.array_equal(dev[k], host[k]) for k in host)


# ---- 11. against the scene generator -------------------------------------------------------------------------------------------------------------------
def test_frustum_of_a_generated_car_holds_the_car_and_the_wall_behind_it(eng):
    from tests.test_tracklet_gpu import _car_box
    mesh = S.load_mesh("builtin", "car", 1)
    eng.scene_upload_meshes([mesh])
    pose = np.array([9.0, 1.0, -1.6, 0.4])
    off = eng.scene_generate([0], [6.0], np.array([[pose, pose]]), sigma=0.0)
    car = eng.scene_read(off)[0]
    assert len(car) > 200
    g = np.random.RandomState(4)
    wall = np.stack([np.full(1500, 25.0) + g.uniform(-0.05, 0.05, 1500), g.uniform(-12, 12, 1500), g.uniform(-2.0, 4.0, 1500)], 1).astype(np.float32)
    frame = BC.pad_stride(np.concatenate([car, wall])[g.permutation(len(car) + len(wall))], 4, g)
    M, image = T.projection(C.KITTI), C.KITTI_IMAGE
    box = _car_box(mesh[0], 6.0, pose)
    rect = C.box_rect(box, M)
    case = dict(scans=[frame], frames=np.zeros((1, 2), np.int32), rects=np.array([[rect, rect]]), proj=M, image=image, dz=np.zeros((1, 2), np.float32), clip=2.0)
    o, p1, p2 = _check(eng, case, "generated scene")
    assert np.array_equal(_bits(p1), _bits(p2))
    crop = {bytes(r) for r in _bits(p1)}
    visible = car[R.inside(car, M, image, C.EVERYWHERE)]
    assert len(visible) > 200 and all(bytes(r) in crop for r in _bits(visible))         # every car return in the image and in front
    n_wall = sum(bytes(r) in crop for r in _bits(wall))
    ob = eng.tracklet_extract(np.zeros((1, 2), np.int32), np.array([[box, box]]))
    b1, _ = eng.tracklet_read(ob)
    print("car returns %d (visible %d), frustum crop %d of which wall %d, box crop %d" % (len(car), len(visible), len(p1), n_wall, len(b1)))
    assert n_wall > 20 and len(p1) == len(visible) + n_wall                             # the background the 3D-box crop does not have
    assert np.array_equal(_bits(b1), _bits(frame[BR.inside(frame, box), :3])) and not any(bytes(r) in {bytes(w) for w in _bits(wall)} for r in _bits(b1))


# ---- 12. the command ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_size", [None, "1242,375"])
def test_make_kitti_dataset_from_bbox2d_end_to_end(gpu_required, tmp_path, image_size):
    """The command in a fresh process on a tiny KITTI-shaped tree with calibration files, labels whose 2D boxes are the projected 3D boxes
    and PNG headers: once reading the headers (the two sequences differ in camera and image size), once with --image-size."""
    kitti, root = tmp_path / "kitti", tmp_path / "KittiTiny"
    C.write_kitti_tree(str(kitti))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    cmd = [sys.executable, os.path.join(PKG, "make_kitti_dataset.py"), "--kitti", str(kitti), "--out", str(root), "--classes", "Car,Pedestrian", "--min-points", "5",
           "--val-seqs", "1", "--from-bbox2d"] + (["--image-size", image_size] if image_size else [])
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    want = []
    for seq in (0, 1):
        labels = T.read_labels(str(kitti / "training" / "label_02" / ("%04d.txt" % seq)))
        M = T.projection(T.read_calib(str(kitti / "training" / "calib" / ("%04d.txt" % seq))))
        for p in T.pairs(labels, ("Car", "Pedestrian"), gap=1, seq=seq):
            scans = [T.read_scan(str(kitti), seq, f) for f in p.frames]
            size = [(1242.0, 375.0) if image_size else T.read_image_size(str(kitti / "training" / "image_02" / ("%04d" % seq) / ("%06d.png" % f))) for f in p.frames]
            l12, zd = T.labels12(p.box1, p.box2)
            c1, c2 = R.crop(scans[0], M, size[0], p.bbox2d1), R.crop(scans[1], M, size[1], p.bbox2d2, np.float32(zd))
            if min(len(c1), len(c2)) >= 5:
                want.append((p, c1, c2))
    n_val = sum(1 for w in want if w[0].seq == 1)
    assert len(want) >= 6 and 0 < n_val < len(want)
    assert "wrote %d pairs (%d train, %d val)" % (len(want), len(want) - n_val, n_val) in r.stdout
    assert [int(x) for x in open(root / "split" / "val.txt").read().split()] == list(range(len(want) - n_val, len(want)))
    assert len(os.listdir(root / "meta")) == len(want)
    for i, (p, c1, c2) in enumerate(want):
        stem = "%08d" % i
        assert json.load(open(root / "meta" / (stem + ".json"))) == json.loads(json.dumps(T.meta(p)))
        for k, c in ((1, c1), (2, c2)):
            pc = np.load(root / ("pointcloud%d" % k) / (stem + ".npy"))
            assert pc.dtype == np.float64 and np.array_equal(pc, c.astype(np.float64)), (i, k)
        assert np.array_equal(np.load(root / "transform" / (stem + ".npy")), T.relative_transform(p.box1, p.box2)[0])
