"""GPU: the ICP kernel's grid search (set_option("icp_search", 1 / 2); csrc/alignnet_icp.hip: icp_grid_build_kernel, icp_kernel<kFull, kTrace, true>)
against the brute-force fp64 restatement with margins of tests/icp_scan_ref.py, on the inputs of tests/icp_grid_ref.py: box-surface clouds above the
scan's LDS budget up to 4 km from the origin, size edges, exact ties on a lattice and the radius on a cell border, one bucket holding 3,000 copies of
a point, clusters 3 km apart, a start 1 km off, radii from a hundredth to fifty times the usual one, mixed batches under the automatic mode, the
drop-in.  Per point through the read-back of ONE evaluation (Engine.debug_icp_grid: the shipped source compiled with a record behind it); whole runs
to the bars of tests/test_icp_scan_gpu.py.  A point within UNDECIDED x b64 of a tie or of the radius is left out of per-point comparisons, a pair with
such a point out of whole-run comparisons; at most POINT_CAP of a test's points may be."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from oracle import alignnet_ref as R
from tests import icp_grid_ref as G
from tests import icp_scan_ref as S
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
SCAN, GRID, AUTO = 0, 1, 2


def _engine(search=GRID):
    eng = alignnet3d.Engine(small_cfg(N=64, nb=12))
    eng.set_option("icp_search", search)
    return eng


@functools.lru_cache(maxsize=None)
def _reference(n2, offset, constrained, its=30):
    """icp_with_margins on the recipe pair, computed once per session and shared."""
    src, dst, _, init = G.box_pair(n2, offset)
    return S.icp_with_margins(src, dst, init, G.RADIUS, its, constrained)


def _read_back(eng, name, src, dst, T, radius, tally, exact=False):
    """One evaluation per point: the grid read-back against the restatement.  Returns (restatement, read-back)."""
    e = S.evaluate_with_margins(src, dst, T, radius, exact=exact)
    edge = G.cell_edge(dst, radius)
    near27, within, lost = G.neighbour_counts(e["p"], dst, edge, radius * (1.0 - 1e-9))   # (1e-9: far above b64 / d, so "within" holds for the kernel's T p too)
    assert not lost.any()
    ok = ~e["undecided"]
    tally[0] += int((~ok).sum()); tally[1] += len(src)
    for constrained in (True, False):
        d = eng.debug_icp_grid(src, dst, T, radius=radius, constrained=constrained)
        bound = 0.0 if exact else S.b64(e["P64"], e["best"])
        inl = ok & e["inlier"]
        err = np.abs(d["dist2"] - e["best"])
        print("%s constrained %d: %d points, %d undecided, fitness %.4f, edge %.9g, buckets occupied %d, largest %d, candidates mean %.1f max %d (in the 27 cells: mean %.1f), "
              "worst distance error over inliers %.3g" % (name, constrained, len(src), (~ok).sum(), d["fitness"], d["cell_edge"], d["buckets_occupied"], d["largest_bucket"],
                                                          d["candidates"].mean() if len(src) else 0, d["candidates"].max() if len(src) else 0,
                                                          near27.mean() if len(src) else 0, err[inl].max() if inl.any() else 0.0))
        assert d["cell_edge"] == edge and d["cell_edge"] > radius, (name, d["cell_edge"], edge)
        bad = np.flatnonzero(inl & (d["index"] != e["index"]))
        assert bad.size == 0, (name, "wrong target for decided inliers", bad[:8], d["index"][bad[:8]], e["index"][bad[:8]])
        assert np.array_equal(d["inlier"][ok], e["inlier"][ok]), name
        # every distance: an inlier's is the restatement's; beyond the radius the nearest CANDIDATE is reported, never nearer than the nearest target
        assert np.all(err[e["inlier"]] <= (bound if exact else bound[e["inlier"]])), name
        assert np.all(d["dist2"] >= e["best"] - bound), name
        assert np.array_equal(d["index"] == -1, d["candidates"] == 0) or len(dst) == 0, name
        assert np.array_equal(np.isinf(d["dist2"]), d["index"] == -1), name
        assert np.all(d["candidates"] >= within), (name, "fewer candidates than targets within the radius")
        if len(dst):
            assert 1 <= d["buckets_occupied"] <= len(dst) and d["largest_bucket"] * d["buckets_occupied"] >= len(dst), name
        if ok.all():   # (rmse: 1e-12 near the origin, 1e-9 beyond 50 m as in tests/test_icp_scan_gpu.py -- b64 / (2 rmse) is 6e-12 per point at 4 km)
            far = len(dst) and float(np.abs(dst).max()) > 50.0
            assert d["fitness"] == e["fitness"] and abs(d["rmse"] - e["rmse"]) < (1e-9 if far else 1e-12), (name, d["fitness"], e["fitness"], d["rmse"] - e["rmse"])
        r = eng.icp_refine([src], [dst], [T], radius=radius, its=0, constrained=constrained)      # the shipped instantiation on the same evaluation
        assert r["fitness"][0] == d["fitness"] and r["rmse"][0] == d["rmse"] and r["iterations"][0] == 0 and np.array_equal(r["transforms"][0], np.asarray(T, np.float64))
    return e, d


def _whole(eng, name, srcs, dsts, inits, radius, its, scale=1.0, refs=None, rmse_tol=1e-12, estimates=(True, False)):
    """Whole runs of a batch against icp_with_margins, both estimates.  Returns the results per estimate and the number of pairs left out."""
    out, skipped = {}, 0
    for constrained in estimates:
        res = eng.icp_refine(srcs, dsts, inits, radius=radius, its=its, constrained=constrained)
        out[constrained] = res
        for k in range(len(srcs)):
            info = {}
            T, fit, rmse, it, und, _ = refs[constrained][k] if refs else S.icp_with_margins(srcs[k], dsts[k], inits[k], radius, its, constrained, info=info)
            err = np.abs(res["transforms"][k] - T).max()
            print("%s pair %d (n1 %d n2 %d) constrained %d: fitness %.4f, %d iterations (device %d), %d undecided, transform error %.3g (bar %.3g), rmse error %.3g"
                  % (name, k, len(srcs[k]), len(dsts[k]), constrained, fit, it, res["iterations"][k], und, err, 1e-9 * scale, abs(res["rmse"][k] - rmse)))
            if und:
                skipped += 1
                continue
            if not constrained and info.get("rank2", 1.0) < 1e-9:   # collinear correspondences: the turn about their line is free (tests/test_icp_scan_gpu.py::test_batch_geometry)
                Rm = res["transforms"][k][:3, :3]
                assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rm) - 1) < 1e-12
                continue
            np.testing.assert_allclose(res["transforms"][k], T, rtol=0, atol=1e-9 * scale, err_msg="%s pair %d" % (name, k))
            assert res["fitness"][k] == fit and res["iterations"][k] == it and abs(res["rmse"][k] - rmse) < rmse_tol, (name, k)
    return out, skipped


# ---- 1. read-back against the margins -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", G.RECIPE_OFFSETS)
def test_grid_read_back_against_margins(gpu_required, offset):
    eng = _engine()
    tally = [0, 0]
    for n2 in G.RECIPE_N2:
        src, dst, T, init = G.box_pair(n2, offset)
        _read_back(eng, "box n2 %d offset %s" % (n2, offset), src, dst, init, G.RADIUS, tally)
    assert tally[0] <= S.POINT_CAP * tally[1], tally
    eng.close()


# ---- 2. size edges --------------------------------------------------------------------------------------------------------------------------------
def _size_pair(n1, n2):
    src, dst, init = S.size_pair(max(n1, 1), max(n2, 1), seed=2000 + n1 + 3 * n2)
    return src[:n1], dst[:n2], init


def test_grid_size_edges(gpu_required):
    eng = _engine()
    cases = G.size_cases()
    pairs = [_size_pair(n1, n2) for n1, n2 in cases]
    tally = [0, 0]
    for (n1, n2), (src, dst, init) in zip(cases, pairs):
        if n1 and n2 and (n1 in (1, 65, 1025) or n2 in (1, 64, 4267)):
            _read_back(eng, "n1 %d n2 %d" % (n1, n2), src, dst, init, 0.1, tally)
    assert tally[0] <= S.POINT_CAP * tally[1], tally
    _, skipped = _whole(eng, "sizes", [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], 0.1, 5)
    assert skipped == 0
    d = eng.debug_icp_grid(pairs[3][0], pairs[3][1][:0], pairs[3][2])        # an empty target: nothing chosen, nothing counted
    assert np.all(d["index"] == -1) and not d["inlier"].any() and d["fitness"] == 0.0 and d["rmse"] == 0.0 and d["buckets_occupied"] == 0
    with pytest.raises(RuntimeError):
        eng.debug_icp_grid(pairs[3][0], pairs[3][1], pairs[3][2], radius=0.0)
    eng.close()


# ---- 3. exact ties ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 512.0, 4096.0])
def test_grid_exact_ties_and_radius_on_a_cell_border(gpu_required, offset):
    eng = _engine()
    src, dst, kinds = G.tie_pair(offset)
    tally = [0, 0]
    e, d = _read_back(eng, "ties offset %s" % offset, src, dst, np.eye(4), G.TIE_RADIUS, tally, exact=True)
    assert tally[0] == 0
    d2 = ((src.astype(np.float64)[:, None, :] - dst.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    assert np.array_equal((d2 == d2.min(1, keepdims=True)).sum(1), kinds)     # 2, 4, 8 equidistant targets; 1 for the radius points
    assert np.array_equal(d["index"], e["index"]) and np.array_equal(d["dist2"], e["best"])    # nothing left out: the lowest original index, the exact distance
    edge = kinds == 1
    assert edge.sum() == 108 and np.all(e["best"][edge] == G.TIE_RADIUS ** 2) and d["inlier"][edge].all() and d["inlier"].all()
    cs, ct = G.cells(src[edge], d["cell_edge"]), G.cells(dst[d["index"][edge]], d["cell_edge"])
    assert (np.abs(cs - ct).max(1) == 1).sum() >= 18 and np.abs(cs - ct).max() == 1     # source and target on different sides of a cell border
    eng.close()


# ---- 4. heavy bucket, wide extent, far start ----------------------------------------------------------------------------------------------------
def test_grid_heavy_bucket_wide_extent_and_far_start(gpu_required):
    eng = _engine()
    tally = [0, 0]
    src, dst, init = G.heavy_pair()
    e, d = _read_back(eng, "heavy", src, dst, init, 0.1, tally)
    assert d["largest_bucket"] >= 3000 and d["candidates"].max() >= 3000
    same = np.flatnonzero((dst == dst[e["index"][0]]).all(1))
    assert len(same) == 3000 and e["index"][0] == same[0] and d["index"][0] == same[0]         # 3,000 equal distances: the lowest index
    _, skipped = _whole(eng, "heavy", [src], [dst], [init], 0.1, 30)
    assert skipped == 0
    used = {}
    for wide in (False, True):
        src, dst, init = G.cluster_pair(wide)
        _read_back(eng, "clusters wide %d" % wide, src, dst, init, 0.1, tally)
        # (3 km apart the full-rotation estimate is ill-conditioned -- the turn about the line through the clusters rests on singular values 2e-7 of the
        # largest, so two correct SVDs may differ by 1e-9 rad, 1.5e-6 m at the clusters: only the z-constrained whole run is held to the restatement there)
        _, skipped = _whole(eng, "clusters wide %d" % wide, [src], [dst], [init], 0.1, 30, scale=3000.0 if wide else 1.0, rmse_tol=1e-12 if not wide else 1e-9,
                            estimates=(True,) if wide else (True, False))
        assert skipped == 0
        used[wide] = eng.get_option("icp_grid_ws_bytes")
    print("workspace of a 4,501-point target: %d bytes in one cluster, %d bytes over 3 km" % (used[False], used[True]))
    assert used[True] == used[False] and 0 < used[True] < 4501 * 64
    assert tally[0] <= S.POINT_CAP * tally[1], tally
    # a start 1 km off: no candidate anywhere, nothing estimated, one repeated evaluation ends the run
    src, dst, _, init = G.box_pair(6000, 0.0)
    far = np.array(init); far[:3, 3] += [600.0, -800.0, 0.0]
    d = eng.debug_icp_grid(src, dst, far)
    assert not d["inlier"].any() and d["fitness"] == 0.0 and np.all(d["dist2"] > 1e5)     # (whatever shares the far cells' hash buckets is met and is far)
    for constrained in (True, False):
        T, fit, rmse, it, und, _ = S.icp_with_margins(src, dst, far, 0.1, 30, constrained)
        r = eng.icp_refine([src], [dst], [far], radius=0.1, its=30, constrained=constrained)
        assert fit == 0.0 and und == 0 and np.array_equal(T, far)
        assert r["fitness"][0] == 0.0 and r["rmse"][0] == 0.0 and r["iterations"][0] == it and np.array_equal(r["transforms"][0], far)
    eng.close()


# ---- 5. radii ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1e-3, 0.1, 0.25, 5.0])
def test_grid_radii(gpu_required, radius):
    """One 6,000-point pair 4 km out: at radius 1e-3 the cell edge is what the coordinates' magnitude allows (4096 x 2^-20 > radius: cells clamped), at
    5.0 the 27 cells hold the whole cloud."""
    eng = _engine()
    src, dst, T, init = G.box_pair(6000, 4096.0)
    tally = [0, 0]
    e, d = _read_back(eng, "radius %g" % radius, src, dst, init, radius, tally)
    assert tally[0] <= S.POINT_CAP * tally[1], tally
    if radius == 1e-3:
        assert d["cell_edge"] > 3.9e-3
        e, d = _read_back(eng, "radius %g at the truth" % radius, src, dst, T, radius, tally)     # (at the disturbed start nothing is within a millimetre)
        assert e["inlier"].sum() > 100
    if radius == 5.0:
        assert d["candidates"].min() >= 6000
    _, skipped = _whole(eng, "radius %g" % radius, [src], [dst], [init], radius, 6, scale=4096.0, rmse_tol=1e-9)
    assert skipped <= 1
    eng.close()


# ---- 6. whole runs ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", G.RECIPE_OFFSETS)
def test_grid_whole_runs(gpu_required, offset):
    eng = _engine()
    pairs = [G.box_pair(n2, offset) for n2 in G.RECIPE_N2]
    srcs, dsts, inits = [p[0] for p in pairs], [p[1] for p in pairs], [p[3] for p in pairs]
    refs = {c: [_reference(n2, offset, c) for n2 in G.RECIPE_N2] for c in (True, False)}
    scale = max(1.0, offset)
    grid, skipped = _whole(eng, "box offset %s" % offset, srcs, dsts, inits, G.RADIUS, 30, scale=scale, refs=refs)
    assert skipped == 0
    eng.set_option("icp_search", SCAN)
    for constrained in (True, False):
        scan = eng.icp_refine(srcs, dsts, inits, radius=G.RADIUS, its=30, constrained=constrained)
        g = grid[constrained]
        assert np.array_equal(scan["fitness"], g["fitness"]) and np.array_equal(scan["iterations"], g["iterations"])
        np.testing.assert_allclose(scan["transforms"], g["transforms"], rtol=0, atol=1e-9 * scale)
        assert 0.9 < g["fitness"].min() and g["iterations"].max() < 30
    eng.close()


# ---- 7. automatic mode -----------------------------------------------------------------------------------------------------------------------------
def test_grid_automatic_mode(gpu_required):
    eng = _engine(SCAN)
    small = [S.size_pair(n1, n2, seed=3000 + n1) for n1, n2 in ((257, 700), (513, 4266), (64, 5))]
    big = [G.box_pair(4267, 0.0), G.box_pair(6000, 512.0)]
    srcs = [small[0][0], big[0][0], small[1][0], small[2][0], big[1][0]]
    dsts = [small[0][1], big[0][1], small[1][1], small[2][1], big[1][1]]
    inits = [small[0][2], big[0][3], small[1][2], small[2][2], big[1][3]]
    is_big = [False, True, False, False, True]
    off = np.zeros((6, 2), np.int64)
    off[1:, 0] = np.cumsum([len(s) for s in srcs]); off[1:, 1] = np.cumsum([len(t) for t in dsts])
    eng.upload_dataset(np.concatenate(srcs), np.concatenate(dsts), off, np.zeros((5, 12), np.float32))
    key = lambda r, k: (r["transforms"][k].tobytes(), r["fitness"][k], r["rmse"][k], int(r["iterations"][k]))
    for constrained in (True, False):
        res = {}
        for mode in (SCAN, GRID, AUTO):
            eng.set_option("icp_search", mode)
            assert eng.get_option("icp_search") == mode
            res[mode] = eng.icp_refine(srcs, dsts, inits, radius=0.1, its=30, constrained=constrained)
        for k in range(5):
            assert key(res[AUTO], k) == key(res[GRID if is_big[k] else SCAN], k), (constrained, k)
        assert any(key(res[GRID], k) != key(res[SCAN], k) for k in range(5))     # (the two searches sum in different orders: the comparison above can tell them apart)
        again = eng.icp_refine(srcs, dsts, inits, radius=0.1, its=30, constrained=constrained)
        order = [4, 0, 3, 1, 2]
        rows = eng.icp_refine_rows(order, [inits[i] for i in order], radius=0.1, its=30, constrained=constrained)
        for k in range(5):
            assert key(again, k) == key(res[AUTO], k), (constrained, k)
            assert key(rows, k) == key(res[AUTO], order[k]), (constrained, k)
    with pytest.raises(RuntimeError, match="icp_search must be 0"):
        eng.set_option("icp_search", 3)
    with pytest.raises(RuntimeError, match="icp_search must be 0"):
        eng.set_option("icp_search", -1)
    assert eng.get_option("icp_search") == AUTO
    eng.close()


# ---- 8. the scan beyond its LDS stage (option 0) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n2", [4267, 12801])
def test_scan_beyond_its_lds_stage(gpu_required, n2):
    """Option 0 where the scan walks its fp64 tail from L2 (one target behind the LDS stage; two more stages' worth): the range no earlier test ran whole
    runs in.  A yardstick for later changes of the scan, not of the grid."""
    eng = _engine(SCAN)
    src, dst, T, init = G.box_pair(n2, 0.0)
    e = S.evaluate_with_margins(src, dst, init, G.RADIUS)
    d = eng.debug_icp_scan(src, dst, init, radius=G.RADIUS)
    ok = ~e["undecided"]
    assert (~ok).sum() <= S.POINT_CAP * len(src)
    assert np.array_equal(d["index"][ok], e["index"][ok]) and np.array_equal(d["inlier"][ok], e["inlier"][ok])
    assert np.all(np.abs(d["dist2"] - e["best"])[ok] <= S.UNDECIDED * S.b64(e["P64"], e["best"])[ok])
    assert d["lds_points"] == S.LDS_BUDGET and np.array_equal(d["tail_won"], d["index"] >= S.LDS_BUDGET)
    assert d["tail_won"].sum() >= (1000 if n2 == 12801 else 0)     # (at 4267 one target lies behind the LDS stage)
    _, skipped = _whole(eng, "scan n2 %d" % n2, [src], [dst], [init], G.RADIUS, 30, refs={c: [_reference(n2, 0.0, c)] for c in (True, False)})
    assert skipped == 0
    eng.close()


# ---- 9. the drop-in -------------------------------------------------------------------------------------------------------------------------------------
def _make_dataset(root, n=20, seed=0):
    """tests/test_dropin_gpu.py's tiny dataset with ONE val pair whose target is a dense blob of 40,000 points (above the scan's LDS budget)."""
    rng = np.random.default_rng(seed)
    d = R.synth_pairs(n, 80, seed=seed, dtype=np.float32)
    for sub in ("meta", "pointcloud1", "pointcloud2", "split"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    txt = lambda v: "\n".join("%.18e" % x for x in np.ravel(v)) + "\n"
    for i in range(n):
        meta = {"translation": txt(d["translations"][i]), "rel_angle": float(d["rel_angles"][i, 0]),
                "start_position": txt(d["pc1_centers"][i]), "end_position": txt(d["pc2_centers"][i]),
                "start_angle": float(d["pc1_angles"][i, 0]), "end_angle": float(d["pc2_angles"][i, 0])}
        json.dump(meta, open(os.path.join(root, "meta", "%08d.json" % i), "w"))
        p2 = d["pcs2"][i][: int(rng.integers(40, 80))]
        if i == n - 2:
            p2 = (p2.mean(0) + rng.uniform(-2.0, 2.0, (40000, 3))).astype(np.float32)
        np.save(os.path.join(root, "pointcloud1", "%08d.npy" % i), d["pcs1"][i][: int(rng.integers(40, 80))])
        np.save(os.path.join(root, "pointcloud2", "%08d.npy" % i), p2)
    open(os.path.join(root, "split", "train.txt"), "w").write("\n".join(map(str, range(12))) + "\n")
    open(os.path.join(root, "split", "val.txt"), "w").write("\n".join(map(str, range(12, n))) + "\n")


def test_train_py_refine_icp_with_automatic_search(gpu_required, tmp_path):
    root = tmp_path / "SynthTiny"
    _make_dataset(str(root))
    user = {"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
            "model": {"num_points": 64, "angles": {"num_bins": 12, "accept_inverted_angle": True},
                      "options": {"s1transformer": [[32, 64, 96], [[64, 32], 0.7]], "s2transformer": [[32, 64, 128], [[64, 32], 0.7]],
                                  "embedding": [32, 64, 160], "remaining_transform_prediction": [[64, 32], 0.7]}},
            "training": {"batch_size": 4, "num_epochs": 2, "learning_rate": 0.002}}
    cfgp = tmp_path / "GridRun.json"
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    env.pop("ALIGNNET_ICP_SEARCH", None)

    def run(args):
        r = subprocess.run([sys.executable, os.path.join(PKG, "train.py")] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout + r.stderr

    json.dump(user, open(cfgp, "w"))
    run(["train", "--config", str(cfgp)])
    ref = tmp_path / "logs" / "GridRun" / "val" / "eval000001" / "refined_p2p"
    got = {}
    for search in (None, "auto"):
        if search:
            json.dump(dict(user, evaluation={"icp_search": search}), open(cfgp, "w"))
        # --use_old_results: both runs refine the predictions stored by the training run's evaluation.  (A fresh forward would not do: the drop-in, like
        # the reference, draws each cloud's num_points sample from the unseeded global np.random stream, so two eval_only processes start ICP from
        # different predictions -- seen on the GPU as different angle levels between two runs of this test's first form.)
        out = run(["eval_only", "--config", str(cfgp), "--eval_epoch", "1", "--refineICP", "--use_old_results"])
        assert ("ICP correspondence search: auto" in out) == (search == "auto")
        got[search] = ({k: np.load(ref / ("%s.npy" % k)) for k in ("pred_translations", "pred_angles")}, json.load(open(ref / "eval.json")))

    def levels(ev, path=""):
        if isinstance(ev, dict):
            return {k2: v2 for k, v in ev.items() for k2, v2 in levels(v, path + "/" + k).items()}
        return {path: ev} if "corr_levels" in path else {}

    assert levels(got[None][1]) and levels(got[None][1]) == levels(got["auto"][1])
    for k in ("pred_translations", "pred_angles"):
        assert np.isfinite(got[None][0][k]).all()
        np.testing.assert_allclose(got["auto"][0][k], got[None][0][k], rtol=0, atol=1e-9)
