"""GPU: the spinning-LiDAR scene generator (include/alignnet_hip.h alignnet_scene_*, csrc/alignnet_scene.hip) through the C ABI against the
fp64 restatement tests/scene_ref.py.  Bars: on every ray the restatement decides (its dilated and eroded casts agree; at most 2 per cloud
may not) the same hit or miss and |t_dev - t_ref| <= 1e-9 m, the project's bar for ICP, RANSAC and FGR; the reported triangle re-intersected
by the restatement gives that t with barycentrics >= -1e-9; points = float32(t d) to 4e-6 (two float32 ulps below 32 m: a rounding flip
of a location that agrees to 1e-9), with noise 1e-7 more (device logf / cosf against NumPy's on a term of at most 0.05).  Inputs: tests/scene_cases.py;
tests/test_scene_cpu.py asserts the restatement leaves none of their rays undecided."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from alignnet3d import scenes as S
from oracle import dataset_ref as D
from tests import scene_cases as C
from tests import scene_ref as R
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
T_TOL, B_TOL, P_TOL = 1e-9, 1e-9, 4e-6
LABELS = ("translations", "rel_angles", "pc1_centers", "pc2_centers", "pc1_angles", "pc2_angles")
WIDTH = dict(translations=3, rel_angles=1, pc1_centers=3, pc2_centers=3, pc1_angles=1, pc2_angles=1)


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


def _upload(eng, *meshes):
    eng.scene_upload_meshes([(v, f, S.mesh_centroid(v, f)) for v, f in meshes])


def _colset(first, count):
    return set(R.window_columns(first, count).tolist())


def _check_cast(dev, name):
    """One debug cast against the restatement on the window the device chose.  Returns (hits, undecided)."""
    v, f, scale, pose = C.CASES[name]
    P = R.pose_vertices(v, scale, pose)
    first, count = dev["window"]
    # the window: every column a triangle's azimuth interval reaches, and no more than a column beyond
    tight, loose = R.window(P, f, margin=-0.01), R.window(P, f, margin=1.01)
    assert _colset(*tight) <= _colset(first, count) <= _colset(*loose), (name, dev["window"], tight, loose)
    cols = R.window_columns(first, count)
    ref = C.reference(name)["cast"] if (first, count) == C.reference(name)["window"] else R.cast(P, f, cols, S.sensor_tables())
    outside = np.ones(R.HRES, bool)
    outside[cols] = False
    assert np.all(np.isinf(dev["t"][:, outside])) and np.all(dev["triangle"][:, outside] == -1)
    t, tri = dev["t"][:, cols], dev["triangle"][:, cols]
    dec = ~ref["undecided"]
    hit = dec & np.isfinite(ref["t"])
    err = float(np.abs(t[hit] - ref["t"][hit]).max()) if hit.any() else 0.0
    t_re, bmin = R.reintersect(P, f, tri, cols, S.sensor_tables())
    err_re = float(np.abs(t_re[hit] - t[hit]).max()) if hit.any() else 0.0
    print("%s: window %s, %d rays, %d hits, %d undecided, max |t_dev - t_ref| %.3g, re-intersected %.3g, min barycentric %.3g"
          % (name, dev["window"], 64 * count, int(hit.sum()), int((~dec).sum()), err, err_re, float(bmin[hit].min()) if hit.any() else 0.0))
    assert (~dec).sum() <= 2
    assert np.array_equal(np.isfinite(t)[dec], np.isfinite(ref["t"])[dec])
    assert np.array_equal(tri >= 0, np.isfinite(t))
    assert err <= T_TOL and err_re <= T_TOL
    assert not hit.any() or bmin[hit].min() >= -B_TOL
    return int(hit.sum()), ref


@pytest.mark.parametrize("name", C.CAST_CASES)
def test_cast_matches_restatement(eng, name):
    v, f, scale, pose = C.CASES[name]
    _upload(eng, (v, f))
    dev = eng.debug_scene_cast(0, scale, pose)
    assert dev["lds_triangles"] == 512
    hits, _ = _check_cast(dev, name)
    assert hits > 1000
    if len(f) > 512:      # the car runs through two chunks as shipped; one chunk size more for it
        small = eng.debug_scene_cast(0, scale, pose, lds_triangles=100)
        assert np.array_equal(small["t"], dev["t"]) and np.array_equal(small["triangle"], dev["triangle"]) and small["window"] == dev["window"]


@pytest.mark.parametrize("name", C.EDGE_CASES)
def test_size_edges_and_chunk_sizes(eng, name):
    """1, 63, 64, 65 and 0 triangles, a mesh above the field of view, exact ties, zero-area and edge-on faces; chunks of 512 (shipped), 64 and 17
    triangles -- several chunks and a ragged last one -- give the identical record."""
    v, f, scale, pose = C.CASES[name]
    _upload(eng, (v, f))
    runs = {lds: eng.debug_scene_cast(0, scale, pose, lds_triangles=lds) for lds in (0, 64, 17)}
    assert [runs[k]["lds_triangles"] for k in (0, 64, 17)] == [512, 64, 17]
    for lds in (64, 17):
        assert runs[lds]["window"] == runs[0]["window"]
        assert np.array_equal(runs[lds]["t"], runs[0]["t"]) and np.array_equal(runs[lds]["triangle"], runs[0]["triangle"]), (name, lds)
    dev = runs[0]
    hits, ref = _check_cast(dev, name)
    cols = R.window_columns(*dev["window"])
    if name == "empty":
        assert dev["window"] == (0, 0) and hits == 0
    elif name == "above":
        assert dev["window"][1] > 0 and hits == 0 and np.all(np.isinf(dev["t"]))
    elif name == "duplicate":     # faces 40 .. 59 repeat faces 10 .. 29: equal t, the lower index is reported -- the restatement's argmin
        tri = dev["triangle"][:, cols]
        assert np.array_equal(tri[~ref["undecided"]], ref["triangle"][~ref["undecided"]])
        assert np.isin(tri, np.arange(10, 30)).sum() > 500 and not np.isin(tri, np.arange(40, 60)).any()
    elif name == "zero_area":
        assert hits > 1000 and not np.isin(dev["triangle"], [0, 1, 2]).any()
    elif name == "edge_on":
        assert set(np.unique(dev["triangle"])) >= {-1, 2}
    else:
        assert hits == len(C.reference(name)["rays"]) > 100
    with pytest.raises(alignnet3d.EngineError, match="lds_triangles"):
        eng.debug_scene_cast(0, scale, pose, lds_triangles=513)


@pytest.mark.parametrize("name", C.WRAP_CASES)
def test_windows_that_wrap_and_the_all_column_window(eng, name):
    v, f, scale, pose = C.CASES[name]
    _upload(eng, (v, f))
    dev = eng.debug_scene_cast(0, scale, pose, lds_triangles=17 if name != "over_sensor" else 0)
    hits, _ = _check_cast(dev, name)
    first, count = dev["window"]
    ref = C.reference(name)
    if name == "over_sensor":
        assert (first, count) == (0, R.HRES) and hits == 64 * R.HRES
    else:
        assert first + count > R.HRES and count < 600       # an object on the bearing of +-180 degrees: columns 44xx .. 4499, 0 .. 1xx
        assert np.isfinite(dev["t"][:, 0]).any() and np.isfinite(dev["t"][:, R.HRES - 1]).any()
    # the generated cloud is in ascending RAY order although the window starts at its high columns
    off = eng.scene_generate([0], [scale], [[pose, pose]], sigma=0.0)
    p1, p2 = eng.scene_read(off)
    assert off.tolist() == [[0, 0], [len(ref["rays"])] * 2] and np.array_equal(p1, p2)
    np.testing.assert_allclose(p1, ref["points"], rtol=0, atol=P_TOL)
    # ... which the points show by themselves: row by row (z / range grows with the row), and inside a row by column (the bearing grows)
    rays = ref["rays"]
    elev = p1[:, 2].astype(np.float64) / np.hypot(p1[:, 0], p1[:, 1])
    np.testing.assert_allclose(elev, S.sensor_tables()[2][rays // R.HRES] / 120.0, atol=1e-5)
    bearing = np.rad2deg(np.arctan2(p1[:, 0].astype(np.float64), p1[:, 1]))
    bearing = np.where(bearing > 179.99, bearing - 360.0, bearing)
    np.testing.assert_allclose(bearing, -180.0 + 0.08 * (rays % R.HRES), atol=1e-4)


def _batch_args():
    names = sorted(C.BATCH_MESHES)
    meshes = [C.BATCH_MESHES[n]() for n in names]
    mesh = [names.index(b[0]) for b in C.BATCH]
    return meshes, mesh, [b[1] for b in C.BATCH], [[b[2], b[3]] for b in C.BATCH], [b[4] for b in C.BATCH]


def _compare_batch(off, p1, p2, sigma, seed, tol, scenes=None):
    scenes = range(len(C.BATCH)) if scenes is None else scenes
    for i, k in enumerate(scenes):
        ref = C.batch_reference(k, sigma, seed)
        for w, blob in enumerate((p1, p2)):
            got = blob[off[i, w]:off[i + 1, w]]
            assert len(got) == len(ref[w]["rays"]), (k, w, len(got), len(ref[w]["rays"]))
            if len(got):
                err = float(np.abs(got.astype(np.float64) - ref[w]["points"]).max())
                print("scene %d cloud %d: %d points, max |point - restatement| %.3g" % (k, w + 1, len(got), err))
                assert err <= tol, (k, w, err)


def test_generate_and_read(eng):
    """B = 5 heterogeneous scenes, noise off: a car twice (two scenes share the mesh), a person, an ellipsoid whose first window wraps and
    whose second cloud is empty, a scaled ellipsoid with a scene id beyond 2^32."""
    meshes, mesh, scale, poses, ids = _batch_args()
    _upload(eng, *meshes)
    off = eng.scene_generate(mesh, scale, poses, scene_ids=ids, seed=7, sigma=0.0)
    p1, p2 = eng.scene_read(off)
    assert off.shape == (6, 2) and off[0].tolist() == [0, 0] and np.all(np.diff(off, axis=0) >= 0)
    assert off[3, 1] == off[2, 1] and off[3, 0] > off[2, 0]          # the empty cloud
    _compare_batch(off, p1, p2, 0.0, 0, P_TOL)
    # a scene generated alone, or in another batch, is bit-identical
    for k in (0, 2, 4):
        o1 = eng.scene_generate([mesh[k]], [scale[k]], [poses[k]], scene_ids=[ids[k]], seed=7, sigma=0.0)
        a, b = eng.scene_read(o1)
        assert np.array_equal(a, p1[off[k, 0]:off[k + 1, 0]]) and np.array_equal(b, p2[off[k, 1]:off[k + 1, 1]]), k
    order = [3, 1, 0]
    o2 = eng.scene_generate([mesh[k] for k in order], [scale[k] for k in order], [poses[k] for k in order], scene_ids=[ids[k] for k in order], sigma=0.0)
    a, b = eng.scene_read(o2)
    for i, k in enumerate(order):
        assert np.array_equal(a[o2[i, 0]:o2[i + 1, 0]], p1[off[k, 0]:off[k + 1, 0]]) and np.array_equal(b[o2[i, 1]:o2[i + 1, 1]], p2[off[k, 1]:off[k + 1, 1]])
    # no scenes: an empty result
    o0 = eng.scene_generate([], [], np.zeros((0, 2, 4)))
    assert o0.tolist() == [[0, 0]] and [len(x) for x in eng.scene_read(o0)] == [0, 0]


def test_noise(eng):
    meshes, mesh, scale, poses, ids = _batch_args()
    _upload(eng, *meshes)
    sigma, clip, seed = 0.05, 0.05, 7
    off0 = eng.scene_generate(mesh, scale, poses, scene_ids=ids, seed=seed, sigma=0.0)
    c1, c2 = eng.scene_read(off0)
    off = eng.scene_generate(mesh, scale, poses, scene_ids=ids, seed=seed, sigma=sigma, clip=clip)
    p1, p2 = eng.scene_read(off)
    assert np.array_equal(off, off0)
    _compare_batch(off, p1, p2, sigma, seed, P_TOL + 1e-7)
    assert np.abs(p1 - c1).max() <= clip + P_TOL and np.abs(p2 - c2).max() <= clip + P_TOL and not np.array_equal(p1, c1)
    # the same seed reproduces the clouds bit for bit -- alone as well as in the batch; another seed or scene id gives others
    again = eng.scene_read(eng.scene_generate(mesh, scale, poses, scene_ids=ids, seed=seed, sigma=sigma, clip=clip))
    assert np.array_equal(again[0], p1) and np.array_equal(again[1], p2)
    o1 = eng.scene_generate([mesh[3]], [scale[3]], [poses[3]], scene_ids=[ids[3]], seed=seed, sigma=sigma, clip=clip)
    a, b = eng.scene_read(o1)
    assert np.array_equal(a, p1[off[3, 0]:off[4, 0]]) and np.array_equal(b, p2[off[3, 1]:off[4, 1]])
    other = eng.scene_read(eng.scene_generate(mesh, scale, poses, scene_ids=ids, seed=seed + 1, sigma=sigma, clip=clip))
    assert not np.array_equal(other[0], p1) and np.abs(other[0] - c1).max() <= clip + P_TOL
    moved = eng.scene_read(eng.scene_generate([mesh[3]], [scale[3]], [poses[3]], scene_ids=[ids[3] + 1], seed=seed, sigma=sigma, clip=clip))
    assert not np.array_equal(moved[0], a)
    # strength = max(0.005, sigma |centroid| / 80): the floor is active at 4 m (0.0025 < 0.005), 0.0125 at 20 m; a tight clip is respected
    ev, ef = C.ellipsoid(1)
    _upload(eng, (ev * 0.6, ef))
    poses2 = [[C.polar(4.0, 40.0), C.polar(20.0, -70.0)]]
    clean = eng.scene_read(eng.scene_generate([0], [1.0], poses2, sigma=0.0))
    noisy = eng.scene_read(eng.scene_generate([0], [1.0], poses2, seed=3, sigma=sigma, clip=clip))
    for k, (dist, want) in enumerate(((4.0, 0.005), (20.0, 0.05 * 20.0 / 80.0))):
        d = (noisy[k].astype(np.float64) - clean[k]).ravel()
        assert d.size > 1000
        # the sample standard deviation of n normal draws is within 4 / sqrt(2 n) of sigma at 4 standard errors; float32 rounding of a point at 20 m adds 1e-6
        print("noise at %g m: std %.5f (want %.5f), %d values" % (dist, d.std(), want, d.size))
        assert abs(d.std() - want) <= want * 4.0 / np.sqrt(2.0 * d.size) + 2e-6, (dist, d.std(), want)
        assert abs(d.mean()) <= 4.0 * want / np.sqrt(d.size) + 2e-6
    tight = eng.scene_read(eng.scene_generate([0], [1.0], poses2, seed=3, sigma=sigma, clip=0.004))
    assert np.abs(tight[1] - clean[1]).max() <= 0.004 + P_TOL and np.abs(tight[1] - clean[1]).max() > 0.0039
    with pytest.raises(alignnet3d.EngineError, match="clip"):
        eng.scene_generate([0], [1.0], poses2, sigma=sigma, clip=0.0)


def _read_batch(eng, ptrs, B, N):
    p1, p2, L = ptrs
    a = eng.read_device(p1, B * N * 3).reshape(B, N, 3)
    b = eng.read_device(p2, B * N * 3).reshape(B, N, 3)
    return a, b, {k: eng.read_device(L[k], B * WIDTH[k]).reshape(B, WIDTH[k]) for k in LABELS}


# noise-free scenes of the built-in car with a small motion between the two views: (pose 1, pose 2)
CAR_PAIRS = ((C.polar(7.0, 35.0, yaw=0.4), C.polar(7.2, 37.0, yaw=0.46)), (C.polar(9.0, -100.0, yaw=2.0), C.polar(9.1, -98.5, yaw=1.95)),
             (C.polar(6.0, 170.0, yaw=-1.0), C.polar(6.2, 172.0, yaw=-1.04)))


def test_install_dataset(gpu_required):
    """The generated scenes as the HBM-resident dataset: the device sampler on them equals the oracle's on the host copy (as
    tests/test_dataset_gpu.py holds it: picks, plain points and labels bit-exact, jittered points to 2e-6), and ICP from the true transform
    finds the two views of a car on each other."""
    N = 64
    e = alignnet3d.Engine(small_cfg(N=N, nb=12))
    with pytest.raises(alignnet3d.EngineError, match="nothing generated"):
        e._check(e._lib.alignnet_scene_install_dataset(e._h, None))
    cv, cf = C.car()
    _upload(e, (cv, cf))
    B = len(CAR_PAIRS)
    off = e.scene_generate([0] * B, [4.4] * B, [list(p) for p in CAR_PAIRS], sigma=0.0)
    p1, p2 = e.scene_read(off)
    rel = [S.rot_z4([0, 0, 0], b[3]) @ np.linalg.inv(S.rot_z4([0, 0, 0], a[3])) for a, b in CAR_PAIRS]   # Rz(yaw2 - yaw1)
    truth = []
    for (a, b), Rm in zip(CAR_PAIRS, rel):
        T = Rm.copy()
        T[:3, 3] = np.array(b[:3]) - Rm[:3, :3] @ np.array(a[:3])        # x2 = R2 (s v) + p2 = Rrel (x1 - p1) + p2
        truth.append(T)
    lab = np.array([np.concatenate([T[:3, 3], [b[3] - a[3]], a[:3], b[:3], [a[3], b[3]]]) for (a, b), T in zip(CAR_PAIRS, truth)], np.float32)
    e.scene_install_dataset(lab)
    rows = [2, 0, 1, 0]
    a, b, labs = _read_batch(e, e.sample_batch(rows, seed=77), len(rows), N)
    ra, rb, rl, picks = D.sample_batch((p1, p2), off, lab, rows, N, 77)
    assert np.array_equal(a, ra) and np.array_equal(b, rb) and picks.min() >= 0
    for k in LABELS:
        assert np.array_equal(labs[k], rl[k]), k
    j, jb, _ = _read_batch(e, e.sample_batch(rows, seed=78, jitter_sigma=0.01, jitter_clip=0.05), len(rows), N)
    rj, rjb, _, _ = D.sample_batch((p1, p2), off, lab, rows, N, 78, 0.01, 0.05)
    np.testing.assert_allclose(j, rj, rtol=0, atol=2e-6)
    np.testing.assert_allclose(jb, rjb, rtol=0, atol=2e-6)
    res = e.icp_refine_rows([0, 1, 2], np.array(truth), radius=0.1, its=30, constrained=False)
    print("ICP from the true transform on the installed car scenes: fitness", res["fitness"], "rmse", res["rmse"], "points", np.diff(off, axis=0).tolist())
    assert np.all(res["fitness"] > 0.9), res["fitness"]
    for T, G in zip(res["transforms"], truth):
        assert np.abs(T[:3, 3] - G[:3, 3]).max() < 0.1 and abs(np.arctan2(T[1, 0], T[0, 0]) - np.arctan2(G[1, 0], G[0, 0])) < 0.03
    # a later generate leaves the installed dataset alone (it was copied)
    e.scene_generate([0], [1.0], [[C.polar(15.0, 0.0), C.polar(15.0, 1.0)]], sigma=0.0)
    a2, _, _ = _read_batch(e, e.sample_batch(rows, seed=77), len(rows), N)
    assert np.array_equal(a2, ra)
    e.close()


def test_errors(gpu_required):
    """Bad input is rejected on the host with a message; nothing reaches a kernel."""
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    ev, ef = C.ellipsoid(1)
    pose = [[C.polar(10.0, 0.0), C.polar(10.0, 5.0)]]
    with pytest.raises(alignnet3d.EngineError, match="no meshes uploaded"):
        e.scene_generate([0], [1.0], pose)
    with pytest.raises(alignnet3d.EngineError, match="no meshes uploaded"):
        e.debug_scene_cast(0, 1.0, pose[0][0])
    with pytest.raises(alignnet3d.EngineError, match="nothing generated"):
        e.scene_read(np.zeros((2, 2), np.int64))
    centroid = S.mesh_centroid(ev, ef)      # of the sound mesh: the bad ones have none to compute
    bad = ef.copy()
    bad[7, 1] = len(ev)
    with pytest.raises(alignnet3d.EngineError, match="face 7 of mesh 0 names vertex %d" % len(ev)):
        e.scene_upload_meshes([(ev, bad, centroid)])
    bad[7, 1] = -1
    with pytest.raises(alignnet3d.EngineError, match="face 7"):
        e.scene_upload_meshes([(ev, bad, centroid)])
    nanv = ev.copy()
    nanv[5, 2] = np.nan
    with pytest.raises(alignnet3d.EngineError, match="non-finite vertex 5"):
        e.scene_upload_meshes([(nanv, ef, centroid)])
    with pytest.raises(alignnet3d.EngineError, match="no meshes uploaded"):      # a failed upload leaves no library behind
        e.scene_generate([0], [1.0], pose)
    _upload(e, (ev, ef))
    with pytest.raises(alignnet3d.EngineError, match="mesh 1 out of range"):
        e.scene_generate([1], [1.0], pose)
    with pytest.raises(alignnet3d.EngineError, match="non-finite pose"):
        e.scene_generate([0], [1.0], [[C.polar(10.0, 0.0), (1.0, np.inf, 0.0, 0.0)]])
    with pytest.raises(alignnet3d.EngineError, match="non-finite scale"):
        e.scene_generate([0], [np.nan], pose)
    assert e._lib.alignnet_scene_generate(e._h, None, None, None, None, -1, 0, 0.0, 0.05, None) != 0
    assert b"B out of range" in e._lib.alignnet_last_error(e._h)
    with pytest.raises(alignnet3d.EngineError, match="nothing generated"):      # none of the failures above left a result
        e.scene_read(np.zeros((2, 2), np.int64))
    off = e.scene_generate([0], [1.0], pose, sigma=0.0)                          # ... and the engine still works
    assert off[1, 0] > 500
    e.scene_free_meshes()
    with pytest.raises(alignnet3d.EngineError, match="no meshes uploaded"):
        e.scene_generate([0], [1.0], pose)
    e.close()


def test_make_synth_dataset_end_to_end(gpu_required, tmp_path):
    """The command in a fresh process writes a dataset of built-in cars and persons; train.py's ICP baseline mode then evaluates it."""
    root = tmp_path / "SynthTiny"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    r = subprocess.run([sys.executable, os.path.join(PKG, "make_synth_dataset.py"), "--out", str(root), "--kind", "carspersons", "--meshes", "builtin",
                        "--n-train", "6", "--n-val", "3", "--seed0", "40"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "wrote 9 scenes (6 train, 3 val)" in r.stdout
    assert open(root / "split" / "train.txt").read().split() == [str(i) for i in range(6)] and open(root / "split" / "val.txt").read().split() == ["6", "7", "8"]
    for i in range(9):
        s = S.draw_scene(40 + i, "carspersons")
        meta = json.load(open(root / "meta" / ("%08d.json" % i)))
        assert meta == json.loads(json.dumps(S.scene_meta(s))) and meta["seed"] == 40 + i
        pc1, pc2 = (np.load(root / ("pointcloud%d" % k) / ("%08d.npy" % i)) for k in (1, 2))
        assert pc1.dtype == np.float64 and pc1.shape[1] == 3 and len(pc1) > 50 and len(pc2) > 50
        assert np.array_equal(np.load(root / "transform" / ("%08d.npy" % i)), s.transform.rel_transform)
        # the cloud lies about the drawn position, at the mesh's size
        assert np.linalg.norm(pc1.mean(0)[:2] - s.transform.start_position[:2]) < 0.6 * s.mesh_scale
    cfgp = tmp_path / "icp_SynthTiny_o3_p2p.json"
    json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
               "evaluation": {"special": {"mode": "icp", "icp": {"variant": "p2point", "with_constraint": True}}}}, open(cfgp, "w"))
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "train", "--config", str(cfgp)], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ev = tmp_path / "logs" / "icp_SynthTiny" / "icp_SynthTiny_o3_p2p" / "val" / "eval000000"
    pt, pa = np.load(ev / "pred_translations.npy"), np.load(ev / "pred_angles.npy")
    assert pt.shape == (3, 3) and pa.shape == (3, 1) and np.isfinite(pt).all() and np.isfinite(pa).all()
    assert json.load(open(ev / "eval.json"))["num"] == 3
