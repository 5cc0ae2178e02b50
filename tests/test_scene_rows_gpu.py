"""GPU: the cast by elevation band of the scene generator (alignnet_set_option "scene_rows" = 1, csrc/alignnet_scene.hip stage 2c: a staged
triangle is intersected only with the bands of 8 rows its mask names) under both stagings, against the scan with the option off, which
tests/test_scene_gpu.py holds to the fp64 restatement.  The bar is equality, bit for bit: the same t, triangle and window per ray from the
read-backs, the same offsets and point blobs from alignnet_scene_generate with the noise on.  The masks themselves are held between two bounds per
(tile, band) (tests/scene_rows_ref.py): every triangle the scan's record reports among a cell's rays must have the band's bit, and no more staged
triangles may have it than the restated rule allows at a margin of 1e-5 (the device's is 1e-8), with its every-band thresholds moved by 1 % for
the triangles whose side of a threshold rounding could decide (scene_rows_ref.UPPER_GUARD), over the triangles the staging may hold (the scan's side tests restated with twice the margin; the tile lists' azimuth bound of
tests/scene_bin_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from alignnet3d import scenes as S
from tests import scene_cases as C
from tests import scene_ref as R
from tests import scene_rows_cases as RC
from tests import scene_rows_ref as RR
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
T_TOL = 1e-9


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


def _upload(eng, *meshes, sensor=None):
    eng.scene_upload_meshes([(v, f, S.mesh_centroid(v, f)) for v, f in meshes], sensor=sensor)


def _same_record(a, b):
    return a["window"] == b["window"] and np.array_equal(a["t"], b["t"]) and np.array_equal(a["triangle"], b["triangle"])


@pytest.mark.parametrize("name", RC.OLD_NAMES + RC.NAMES)
def test_band_records_equal_the_scan_and_cell_counts_are_bounded(eng, name):
    v, f, scale, pose = RC.case(name)
    tables = RC.tables(name)
    try:
        _upload(eng, (v, f), sensor=tables)
        scan = eng.debug_scene_cast(0, scale, pose)
        assert "cell_counts" not in scan
        P = R.pose_vertices(v, scale, pose)
        first, count = scan["window"]
        tiles = (count + 7) // 8
        lower = RR.cell_lower(scan["triangle"], scan["window"])
        loose = RR.masks(P, f, scan["window"], tables, margin=RR.UPPER_MARGIN, guard=RR.UPPER_GUARD)
        members = {False: RR.scan_members(P, f, scan["window"], tables), True: RR.list_members(P, f, scan["window"])}
        for binned in (False, True):
            rec = eng.debug_scene_cast(0, scale, pose, binned=binned, rows=True)
            assert rec["lds_triangles"] == 512 and "tile_counts" not in rec
            assert _same_record(rec, scan), (name, binned)
            # chunks of 17 triangles: several chunks and a ragged last one
            small = eng.debug_scene_cast(0, scale, pose, lds_triangles=17, binned=binned, rows=True)
            assert small["lds_triangles"] == 17 and _same_record(small, scan), (name, binned)
            cc = rec["cell_counts"]
            assert cc.shape == (tiles, 8) and rec["cells"] == int(cc.sum())
            assert np.array_equal(small["cell_counts"], cc) and small["cells"] == rec["cells"]
            upper = RR.cell_upper(members[binned], loose)
            print("%s, %s staging: window %s, %d tiles, %d cells with a triangle; set bits %d, reported by the scan %d, allowed %d of %d staged x 8" %
                  (name, "list" if binned else "scan", scan["window"], tiles, int((cc > 0).sum()), rec["cells"], int(lower.sum()), int(upper.sum()),
                   int(members[binned].sum())))
            assert np.all(lower <= cc), (name, binned, np.argwhere(lower > cc)[:10])
            assert np.all(cc <= upper), (name, binned, np.argwhere(cc > upper)[:10])
            if name == "empty":
                assert scan["window"] == (0, 0) and rec["cells"] == 0 and np.all(np.isinf(rec["t"]))
            elif name == "over_and_under":
                assert tiles == 563 and np.all(cc == 2)          # both faces in every cell
            elif name == "above":
                assert rec["cells"] == 0 and np.all(np.isinf(rec["t"]))      # staged for no band at all
            elif name == "car_6m":
                assert 0 < rec["cells"] < 4 * int(members[binned].sum())     # the point of it: well under 8 bands per staged triangle
    finally:
        if name == "custom_sensor":
            _upload(eng, (v, f))      # the default tables again


def test_custom_sensor_matches_the_restatement(eng):
    """Case (e): dir_z a permutation (bands of unrelated rows), column norms from 84 to 156.  Equal to scene_rows = 0 bit for bit under both
    stagings and through alignnet_scene_generate, and equal to the restatement's cast with those tables on its decided rays to 1e-9."""
    v, f, scale, pose = RC.case("custom_sensor")
    tables = RC.sensor()
    try:
        _upload(eng, (v, f), sensor=tables)
        scan = eng.debug_scene_cast(0, scale, pose)
        first, count = scan["window"]
        cols = R.window_columns(first, count)
        ref = R.cast(R.pose_vertices(v, scale, pose), f, cols, tables)
        dec = ~ref["undecided"]
        hit = dec & np.isfinite(ref["t"])
        assert hit.sum() > 5000 and (~dec).sum() <= 2
        for binned in (False, True):
            rec = eng.debug_scene_cast(0, scale, pose, binned=binned, rows=True)
            assert _same_record(rec, scan)
            t = rec["t"][:, cols]
            assert np.array_equal(np.isfinite(t)[dec], np.isfinite(ref["t"])[dec])
            err = float(np.abs(t[hit] - ref["t"][hit]).max())
            print("custom sensor, %s staging: %d hits, max |t_dev - t_ref| %.3g" % ("list" if binned else "scan", int(hit.sum()), err))
            assert err <= T_TOL
            assert np.array_equal(rec["triangle"][:, cols][hit], ref["triangle"][hit])
        res = {}
        for cast in (0, 1):
            for rows in (0, 1):
                eng.set_option("scene_cast", cast); eng.set_option("scene_rows", rows)
                off = eng.scene_generate([0], [scale], [[pose, pose]], seed=3, sigma=0.05, clip=0.05)
                res[cast, rows] = (off, *eng.scene_read(off))
        for key, (off, p1, p2) in res.items():
            assert np.array_equal(off, res[0, 0][0]) and np.array_equal(p1, res[0, 0][1]) and np.array_equal(p2, res[0, 0][2]), key
        assert res[0, 0][0][-1, 0] == np.isfinite(scan["t"]).sum()
    finally:
        eng.set_option("scene_cast", 0); eng.set_option("scene_rows", 0)
        _upload(eng, (v, f))


def _batch_args():
    names = sorted(C.BATCH_MESHES)
    meshes = [C.BATCH_MESHES[n]() for n in names]
    mesh = [names.index(b[0]) for b in C.BATCH]
    return meshes, mesh, [b[1] for b in C.BATCH], [[b[2], b[3]] for b in C.BATCH], [b[4] for b in C.BATCH]


def test_generate_is_bit_identical_under_all_six_settings(eng):
    meshes, mesh, scale, poses, ids = _batch_args()
    _upload(eng, *meshes)
    kw = dict(seed=7, sigma=0.05, clip=0.05)
    res = {}
    try:
        for cast in (0, 1, 2):
            for rows in (0, 1):
                eng.set_option("scene_cast", cast); eng.set_option("scene_rows", rows)
                off = eng.scene_generate(mesh, scale, poses, scene_ids=ids, **kw)
                res[cast, rows] = (off, *eng.scene_read(off), eng.get_option("scene_binned_clouds"))
        assert [res[c, 1][3] for c in (0, 1, 2)] == [0, 10, 4]      # which clouds are binned does not depend on scene_rows
        assert res[0, 0][0][-1].min() > 1000
        for key, r in res.items():
            assert np.array_equal(r[0], res[0, 0][0]), key
            assert np.array_equal(r[1], res[0, 0][1]) and np.array_equal(r[2], res[0, 0][2]), key
        off, p1, p2 = res[0, 0][:3]
        for cast in (0, 1):
            eng.set_option("scene_cast", cast); eng.set_option("scene_rows", 1)
            for k in (0, 2):      # a car; a wrapped window with an empty second cloud -- alone
                o1 = eng.scene_generate([mesh[k]], [scale[k]], [poses[k]], scene_ids=[ids[k]], **kw)
                a, b = eng.scene_read(o1)
                assert np.array_equal(a, p1[off[k, 0]:off[k + 1, 0]]) and np.array_equal(b, p2[off[k, 1]:off[k + 1, 1]]), (cast, k)
            for _ in range(2):    # two calls in a row
                again = eng.scene_generate(mesh, scale, poses, scene_ids=ids, **kw)
                q1, q2 = eng.scene_read(again)
                assert np.array_equal(again, off) and np.array_equal(q1, p1) and np.array_equal(q2, p2), cast
    finally:
        eng.set_option("scene_cast", 0); eng.set_option("scene_rows", 0)


def test_option_handling(eng):
    assert eng.get_option("scene_rows") == 0
    fresh = alignnet3d.Engine(small_cfg(N=64, nb=12))
    assert fresh.get_option("scene_rows") == 0 and fresh.get_option("scene_cast") == 0
    fresh.close()
    try:
        for keep in (1, 0):
            eng.set_option("scene_rows", keep)
            for bad in (2, -1, 255):
                with pytest.raises(alignnet3d.EngineError, match="scene_rows must be 0"):
                    eng.set_option("scene_rows", bad)
                assert eng.get_option("scene_rows") == keep
        eng.set_option("scene_rows", 1)
        with pytest.raises(alignnet3d.EngineError, match="scene_cast must be 0"):
            eng.set_option("scene_cast", 3)
        assert eng.get_option("scene_rows") == 1 and eng.get_option("scene_cast") == 0
        # the read-backs take their own path whatever the options say
        v, f, scale, pose = C.CASES["first65"]
        _upload(eng, (v, f))
        eng.set_option("scene_cast", 1)
        plain = eng.debug_scene_cast(0, scale, pose)
        assert "cell_counts" not in plain and "tile_counts" not in plain
        assert "tile_counts" in eng.debug_scene_cast(0, scale, pose, binned=True)
        eng.set_option("scene_rows", 0); eng.set_option("scene_cast", 0)
        rec = eng.debug_scene_cast(0, scale, pose, binned=True, rows=True)
        assert rec["cells"] > 0 and _same_record(rec, plain)
        assert eng.get_option("scene_rows") == 0 and eng.get_option("scene_cast") == 0
        with pytest.raises(alignnet3d.EngineError, match=r"lds_triangles must be in \[0, 512\]"):
            eng.debug_scene_cast(0, scale, pose, lds_triangles=513, rows=True)
    finally:
        eng.set_option("scene_cast", 0); eng.set_option("scene_rows", 0)


def test_make_synth_dataset_writes_the_same_files_with_rows(gpu_required, tmp_path):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    roots = {}
    for rows in (False, True):
        roots[rows] = tmp_path / ("rows" if rows else "plain")
        r = subprocess.run([sys.executable, os.path.join(PKG, "make_synth_dataset.py"), "--out", str(roots[rows]), "--meshes", "builtin",
                            "--kind", "carspersons", "--n-train", "4", "--n-val", "2", "--seed0", "40"] + (["--rows"] if rows else []),
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "wrote 6 scenes (4 train, 2 val)" in r.stdout
        assert ("cast scan (0 of 12 clouds binned)" + (" by elevation band" if rows else ",")) in r.stdout, r.stdout
    for i in range(6):
        for sub in ("pointcloud1", "pointcloud2", "transform"):
            a, b = (np.load(roots[k] / sub / ("%08d.npy" % i)) for k in (False, True))
            assert a.dtype == b.dtype and np.array_equal(a, b), (sub, i)
            assert sub == "transform" or len(a) > 50
        assert open(roots[False] / "meta" / ("%08d.json" % i)).read() == open(roots[True] / "meta" / ("%08d.json" % i)).read()
    for name in ("train.txt", "val.txt"):
        assert open(roots[False] / "split" / name).read() == open(roots[True] / "split" / name).read()
