"""GPU: the binned cast of the scene generator (alignnet_set_option "scene_cast" = 1 / 2, csrc/alignnet_scene.hip: triangles binned to the 8-column
tiles of a cloud's window, a tile casting only its own list) against the scan (option 0), which tests/test_scene_gpu.py holds to the fp64
restatement.  The bar is equality, bit for bit: the same t, triangle and window per ray from the read-backs, the same offsets and point blobs from
alignnet_scene_generate with the noise on.  The tile lists themselves are held between two bounds (tests/scene_bin_ref.py): every triangle the
scan's record reports among a tile's columns must be on its list, and no triangle whose azimuth interval, dilated by 1.01 columns, stays clear
of the tile may be."""
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from alignnet3d import scenes as S
from tests import scene_bin_ref as BR
from tests import scene_cases as C
from tests import scene_ref as R
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
T_TOL, B_TOL = 1e-9, 1e-9
NAMES = C.CAST_CASES + C.EDGE_CASES + C.WRAP_CASES


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


def _upload(eng, *meshes):
    eng.scene_upload_meshes([(v, f, S.mesh_centroid(v, f)) for v, f in meshes])


def _same_record(a, b):
    return a["window"] == b["window"] and np.array_equal(a["t"], b["t"]) and np.array_equal(a["triangle"], b["triangle"])


@pytest.mark.parametrize("name", NAMES)
def test_binned_record_equals_the_scan_and_lists_are_sufficient_and_not_loose(eng, name):
    v, f, scale, pose = C.CASES[name]
    _upload(eng, (v, f))
    scan = eng.debug_scene_cast(0, scale, pose)
    binned = eng.debug_scene_cast(0, scale, pose, binned=True)
    assert "tile_counts" not in scan and binned["lds_triangles"] == 512
    assert _same_record(binned, scan), name
    # chunks of 17 triangles: several chunks and a ragged last one inside a tile's list
    small = eng.debug_scene_cast(0, scale, pose, lds_triangles=17, binned=True)
    assert small["lds_triangles"] == 17 and _same_record(small, scan), name
    assert np.array_equal(small["tile_counts"], binned["tile_counts"]) and small["entries"] == binned["entries"]
    first, count = scan["window"]
    counts = binned["tile_counts"]
    assert counts.shape == (BR.tiles_of(count),) and binned["entries"] == int(counts.sum())
    lower = BR.lower_bound(scan["triangle"], scan["window"])
    upper = BR.upper_bound(R.pose_vertices(v, scale, pose), f, scan["window"])
    print("%s: window %s, %d tiles, %d entries, longest list %d; reported by the scan %d, allowed %d" %
          (name, scan["window"], len(counts), binned["entries"], int(counts.max()) if len(counts) else 0, int(lower.sum()), int(upper.sum())))
    assert np.all(lower <= counts), (name, np.flatnonzero(lower > counts)[:10])
    assert np.all(counts <= upper), (name, np.flatnonzero(counts > upper)[:10])
    cols = R.window_columns(first, count)
    if name == "empty":
        assert scan["window"] == (0, 0) and binned["entries"] == 0 and len(counts) == 0 and np.all(np.isinf(binned["t"]))
    elif name == "over_sensor":
        assert len(counts) == 563 and counts.min() > 0
    elif name == "duplicate":
        tri = binned["triangle"][:, cols]
        assert np.isin(tri, np.arange(10, 30)).sum() > 500 and not np.isin(tri, np.arange(40, 60)).any()
    elif name in ("ellipsoid80_12m", "ellipsoid320_12m", "car_6m"):
        assert counts.max() > 17                      # (the 17-triangle chunks above did split a list)


def _check_record(dev, v, f, scale, pose):
    """A read-back against the restatement on the window the device chose, as tests/test_scene_gpu.py holds the scan.  Returns the hits."""
    P = R.pose_vertices(v, scale, pose)
    first, count = dev["window"]
    colset = lambda w: set(R.window_columns(*w).tolist())
    assert colset(R.window(P, f, margin=-0.01)) <= colset((first, count)) <= colset(R.window(P, f, margin=1.01))
    cols = R.window_columns(first, count)
    ref = R.cast(P, f, cols, S.sensor_tables())
    outside = np.ones(R.HRES, bool)
    outside[cols] = False
    assert np.all(np.isinf(dev["t"][:, outside])) and np.all(dev["triangle"][:, outside] == -1)
    t, tri = dev["t"][:, cols], dev["triangle"][:, cols]
    dec = ~ref["undecided"]
    hit = dec & np.isfinite(ref["t"])
    err = float(np.abs(t[hit] - ref["t"][hit]).max()) if hit.any() else 0.0
    t_re, bmin = R.reintersect(P, f, tri, cols, S.sensor_tables())
    err_re = float(np.abs(t_re[hit] - t[hit]).max()) if hit.any() else 0.0
    print("window %s, %d hits, %d undecided, max |t_dev - t_ref| %.3g, re-intersected %.3g" % (dev["window"], int(hit.sum()), int((~dec).sum()), err, err_re))
    assert (~dec).sum() <= 2
    assert np.array_equal(np.isfinite(t)[dec], np.isfinite(ref["t"])[dec])
    assert np.array_equal(tri >= 0, np.isfinite(t))
    assert err <= T_TOL and err_re <= T_TOL
    assert not hit.any() or bmin[hit].min() >= -B_TOL
    return int(hit.sum()), int((~dec).sum())


def test_empty_tiles_inside_a_window(eng):
    """Two small ellipsoids side by side: one window of 47 tiles, 25 of which no triangle reaches -- workgroups with an empty list."""
    v, f, scale, pose = BR.case("two_blobs")
    _upload(eng, (v, f))
    scan = eng.debug_scene_cast(0, scale, pose)
    binned = eng.debug_scene_cast(0, scale, pose, binned=True)
    assert _same_record(binned, scan)
    assert binned["window"] == (2779, 372) and len(binned["tile_counts"]) == 47
    hits, undecided = _check_record(binned, v, f, scale, pose)
    assert hits == 1380 and undecided == 0
    counts = binned["tile_counts"]
    assert (counts == 0).sum() >= 20 and counts[0] > 0 and counts[-1] > 0
    assert np.all(BR.lower_bound(scan["triangle"], scan["window"]) <= counts) and np.all(counts <= BR.upper_bound(R.pose_vertices(v, scale, pose), f, scan["window"]))
    # the rays of the empty tiles miss
    cols = R.window_columns(*binned["window"])
    for k in np.flatnonzero(counts == 0):
        assert np.all(np.isinf(binned["t"][:, cols[k * 8:(k + 1) * 8]]))


def test_more_triangles_than_one_pass_and_one_chunk(eng):
    """2,064 triangles: every thread of the tally and the fill takes several, and the scan needs five LDS chunks."""
    v, f = BR.car2064()
    scale, pose = 6.0, C.polar(8.0, 100.0, yaw=0.7)
    _upload(eng, (v, f))
    scan = eng.debug_scene_cast(0, scale, pose)
    assert np.isfinite(scan["t"]).sum() > 5000
    P = R.pose_vertices(v, scale, pose)
    reaching = int((BR.triangle_intervals(P, f, 1e-6)[0] != 0).sum())      # every triangle of non-zero area is on at least one list
    upper = BR.upper_bound(P, f, scan["window"])
    for lds in (0, 100):
        binned = eng.debug_scene_cast(0, scale, pose, lds_triangles=lds, binned=True)
        assert _same_record(binned, scan), lds
        assert binned["entries"] == int(binned["tile_counts"].sum()) and reaching <= binned["entries"] <= int(upper.sum())
        assert np.all(binned["tile_counts"] <= upper)
    print("car2064 at 8 m: window %s, %d entries for %d triangles, longest list %d" % (scan["window"], binned["entries"], len(f), int(binned["tile_counts"].max())))
    assert reaching > 2000 and binned["tile_counts"].max() > 200      # lists of several 100-triangle chunks (252 by the window kernel's rule on the CPU)


def _batch_args():
    names = sorted(C.BATCH_MESHES)
    meshes = [C.BATCH_MESHES[n]() for n in names]
    mesh = [names.index(b[0]) for b in C.BATCH]
    return meshes, mesh, [b[1] for b in C.BATCH], [[b[2], b[3]] for b in C.BATCH], [b[4] for b in C.BATCH]


def test_generate_is_bit_identical_under_every_option(eng):
    meshes, mesh, scale, poses, ids = _batch_args()
    _upload(eng, *meshes)
    kw = dict(seed=7, sigma=0.05, clip=0.05)
    res = {}
    try:
        for opt in (0, 1, 2):
            eng.set_option("scene_cast", opt)
            off = eng.scene_generate(mesh, scale, poses, scene_ids=ids, **kw)
            res[opt] = (off, *eng.scene_read(off), eng.get_option("scene_binned_clouds"))
        assert [res[o][3] for o in (0, 1, 2)] == [0, 10, 4]      # auto: only the car (516 triangles) exceeds 512, scenes 0 and 3
        assert res[0][0][-1].min() > 1000
        for opt in (1, 2):
            assert np.array_equal(res[opt][0], res[0][0]), opt
            assert np.array_equal(res[opt][1], res[0][1]) and np.array_equal(res[opt][2], res[0][2]), opt
        eng.set_option("scene_cast", 1)
        off, p1, p2 = res[1][:3]
        o1 = eng.scene_generate([mesh[2]], [scale[2]], [poses[2]], scene_ids=[ids[2]], **kw)      # a wrapped window and an empty cloud, alone
        a, b = eng.scene_read(o1)
        assert eng.get_option("scene_binned_clouds") == 2
        assert np.array_equal(a, p1[off[2, 0]:off[3, 0]]) and np.array_equal(b, p2[off[2, 1]:off[3, 1]]) and len(b) == 0
        # the fill hands out list slots by atomics: the order inside a list may differ between calls, the clouds may not
        for _ in range(2):
            again = eng.scene_generate(mesh, scale, poses, scene_ids=ids, **kw)
            q1, q2 = eng.scene_read(again)
            assert np.array_equal(again, off) and np.array_equal(q1, p1) and np.array_equal(q2, p2)
    finally:
        eng.set_option("scene_cast", 0)


def test_option_handling(eng):
    assert eng.get_option("scene_cast") == 0
    fresh = alignnet3d.Engine(small_cfg(N=64, nb=12))
    assert fresh.get_option("scene_cast") == 0 and fresh.get_option("scene_binned_clouds") == 0
    fresh.close()
    try:
        eng.set_option("scene_cast", 2)
        for bad in (3, -1):
            with pytest.raises(alignnet3d.EngineError, match="scene_cast must be 0"):
                eng.set_option("scene_cast", bad)
            assert eng.get_option("scene_cast") == 2
    finally:
        eng.set_option("scene_cast", 0)
    v, f, scale, pose = C.CASES["first65"]
    _upload(eng, (v, f))
    with pytest.raises(alignnet3d.EngineError, match=r"lds_triangles must be in \[0, 512\]"):
        eng.debug_scene_cast(0, scale, pose, lds_triangles=513, binned=True)
    with pytest.raises(alignnet3d.EngineError, match="lds_triangles"):
        eng.debug_scene_cast(0, scale, pose, lds_triangles=-1, binned=True)
    # the read-backs choose their own path whatever the option says
    try:
        eng.set_option("scene_cast", 1)
        assert "tile_counts" not in eng.debug_scene_cast(0, scale, pose)
    finally:
        eng.set_option("scene_cast", 0)
    assert eng.debug_scene_cast(0, scale, pose, binned=True)["entries"] > 0


def test_make_synth_dataset_writes_the_same_files_binned(gpu_required, tmp_path):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    roots = {}
    for cast in ("scan", "binned"):
        roots[cast] = tmp_path / cast
        r = subprocess.run([sys.executable, os.path.join(PKG, "make_synth_dataset.py"), "--out", str(roots[cast]), "--cast", cast, "--meshes", "builtin",
                            "--kind", "carspersons", "--n-train", "4", "--n-val", "2", "--seed0", "40"], cwd=str(tmp_path), env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "wrote 6 scenes (4 train, 2 val)" in r.stdout
        assert ("cast %s (%d of 12 clouds binned)" % (cast, 12 if cast == "binned" else 0)) in r.stdout, r.stdout
    for i in range(6):
        for sub in ("pointcloud1", "pointcloud2", "transform"):
            a, b = (np.load(roots[c] / sub / ("%08d.npy" % i)) for c in ("scan", "binned"))
            assert a.dtype == b.dtype and np.array_equal(a, b), (sub, i)
            assert sub == "transform" or len(a) > 50
        assert open(roots["scan"] / "meta" / ("%08d.json" % i)).read() == open(roots["binned"] / "meta" / ("%08d.json" % i)).read()
    for name in ("train.txt", "val.txt"):
        assert open(roots["scan"] / "split" / name).read() == open(roots["binned"] / "split" / name).read()
