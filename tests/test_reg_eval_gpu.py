"""GPU: alignnet_evaluate_registration* (csrc/alignnet_icp.hip, icp_kernel<false, false, kGrid, true>) against its definition in
tests/reg_eval_ref.py, under the scan and the grid search: size edges (both empty kinds, the ends of the kernel's rounds, a target behind the scan's
LDS stage), the threshold hit exactly and missed by one ulp, 4-way exact ties, a pair 4 km out with and without a centre, thresholds from 1 mm to
5 m, a mixed batch bit-identical to its pairs alone and through the dataset entry, Engine.icp_refine(its=0) as a second opinion, the entry points'
errors, and train.py with evaluation.reg_eval.

Bars: correspondences equal on every decided point (the committed inputs have no undecided one, tests/test_reg_eval_cpu.py); fitness equal; rmse
within 1e-12 relative; the information matrix within 1e-9 of its largest diagonal entry (the bar the project holds ICP transforms to) and symmetric
bit for bit.  Against icp_refine(its=0) -- another instantiation of the same source, which the compiler may fuse differently -- fitness is equal and
rmse is held to the same 1e-12."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import alignnet3d
from tests import reg_eval_ref as R
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
SCAN, GRID = 0, 1
RMSE_BAR, INFO_BAR = 1e-12, 1e-9


@functools.lru_cache(maxsize=None)
def _cases():
    return {c["name"]: c for c in R.all_cases()}


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The restatement of a committed case, computed once per session and shared (never modified)."""
    c = _cases()[name]
    return R.evaluate_registration(c["src"], c["dst"], c["T"], c["threshold"], c["centre"], c["exact"])


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


def _call(eng, names, search, rows=None):
    cs = [_cases()[n] for n in names]
    assert len({c["threshold"] for c in cs}) == 1
    eng.set_option("icp_search", search)
    centres = None if all(c["centre"] is None for c in cs) else [np.zeros(3) if c["centre"] is None else c["centre"] for c in cs]
    kw = dict(threshold=cs[0]["threshold"], centers=centres, want_information=True, want_correspondences=True)
    if rows is not None:
        return eng.evaluate_registration_rows(rows, [c["T"] for c in cs], **kw)
    return eng.evaluate_registration([c["src"] for c in cs], [c["dst"] for c in cs], [c["T"] for c in cs], **kw)


def _same(a, b, i=0, j=0):
    """two results of the device bit for bit"""
    return (a["fitness"][i] == b["fitness"][j] and a["rmse"][i] == b["rmse"][j] and np.array_equal(a["information"][i], b["information"][j])
            and np.array_equal(a["correspondences"][i], b["correspondences"][j]))


def _check(name, got, i, worst):
    ref = _ref(name)
    ok = ~ref["undecided"]
    assert (~ok).sum() <= R.POINT_CAP * max(len(ok), 1), name
    corr, info = got["correspondences"][i], got["information"][i]
    assert corr.dtype == np.int32 and corr.shape == ref["correspondences"].shape, name
    bad = np.flatnonzero(ok & (corr != ref["correspondences"]))
    assert bad.size == 0, (name, bad[:5], corr[bad[:5]], ref["correspondences"][bad[:5]])
    if ok.all():
        assert got["fitness"][i] == ref["fitness"], (name, got["fitness"][i], ref["fitness"])
        rel = abs(got["rmse"][i] - ref["rmse"]) / ref["rmse"] if ref["rmse"] else abs(got["rmse"][i])
        scale = ref["information"].diagonal().max()
        gap = np.abs(info - ref["information"]).max() / scale if scale else np.abs(info).max()
        worst[0], worst[1] = max(worst[0], rel), max(worst[1], gap)
        assert rel <= RMSE_BAR, (name, got["rmse"][i], ref["rmse"])
        assert gap <= INFO_BAR, (name, gap)
    assert np.array_equal(info, info.T), name
    assert np.isfinite(info).all() and np.isfinite(got["rmse"][i]), name


def _agree(name, a, b):
    """scan and grid on one pair: same correspondences and fitness, rmse / information within the bars"""
    assert np.array_equal(a["correspondences"][0], b["correspondences"][0]) and a["fitness"][0] == b["fitness"][0], name
    assert abs(a["rmse"][0] - b["rmse"][0]) <= RMSE_BAR * max(a["rmse"][0], 1e-300), name
    scale = max(a["information"][0].diagonal().max(), 1e-300)
    assert np.abs(a["information"][0] - b["information"][0]).max() <= INFO_BAR * scale, name


def _each(eng, names, label):
    worst = [0.0, 0.0]
    for name in names:
        got = {s: _call(eng, [name], s) for s in (SCAN, GRID)}
        for s in (SCAN, GRID):
            _check(name, got[s], 0, worst)
        _agree(name, got[SCAN], got[GRID])
    print("%s: %d pairs x (scan, grid): worst rmse gap %.3g relative, worst information gap %.3g of the largest diagonal entry" % (label, len(names), worst[0], worst[1]))


def test_size_edges(eng):
    names = [c["name"] for c in R.size_cases()]
    assert len(names) == len(R.SIZES_N1) * len(R.SIZES_N2) + len(R.SIZES_TAIL)
    _each(eng, names, "size edges")
    # the empty kinds in full: nothing but zeros and -1
    for name in ("size_0_5", "size_257_0", "size_0_0"):
        g = _call(eng, [name], SCAN)
        assert g["fitness"][0] == 0.0 and g["rmse"][0] == 0.0 and not g["information"][0].any() and (g["correspondences"][0] == -1).all()
    # a target behind the scan's LDS stage is found
    assert _call(eng, ["size_257_%d" % (R.LDS_BUDGET + 1)], SCAN)["correspondences"][0][0] == R.LDS_BUDGET


def test_threshold_hit_exactly_and_missed_by_one_ulp(eng):
    _each(eng, ["threshold_edge"], "threshold edge")
    _, per = R.threshold_edge_case()
    for s in (SCAN, GRID):
        c = _call(eng, ["threshold_edge"], s)["correspondences"][0]
        assert (c[:2 * per] >= 0).all() and (c[2 * per:] == -1).all()


def test_four_way_exact_ties(eng):
    _each(eng, ["ties4"], "4-way ties")


def test_far_frame_with_and_without_a_centre(eng):
    _each(eng, ["far_origin", "far_centred"], "4 km out")


def test_threshold_range(eng):
    _each(eng, ["threshold_%g" % t for t in R.THRESHOLDS], "thresholds")


def test_icp_refine_with_no_iteration_is_the_same_evaluation(eng):
    for name in ("size_257_5", "size_257_%d" % (R.LDS_BUDGET + 1), "far_origin", "threshold_0.02", "threshold_5", "ties4"):
        c = _cases()[name]
        for s in (SCAN, GRID):
            got = _call(eng, [name], s)
            icp = eng.icp_refine([c["src"]], [c["dst"]], [c["T"]], radius=c["threshold"], its=0)
            assert icp["iterations"][0] == 0 and np.array_equal(icp["transforms"][0], c["T"])
            print("%s search %d: fitness %.6f, rmse %.17g (evaluate) %.17g (icp_refine its=0)" % (name, s, got["fitness"][0], got["rmse"][0], icp["rmse"][0]))
            assert icp["fitness"][0] == got["fitness"][0]
            assert abs(icp["rmse"][0] - got["rmse"][0]) <= RMSE_BAR * got["rmse"][0]


def test_batch_equals_its_pairs_alone_and_the_dataset_entry(eng):
    cases = R.batch_cases()
    names = [c["name"] for c in cases]
    off = np.zeros((len(cases) + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(c["src"]) for c in cases]); off[1:, 1] = np.cumsum([len(c["dst"]) for c in cases])
    eng.upload_dataset(np.concatenate([c["src"] for c in cases]), np.concatenate([c["dst"] for c in cases]), off, np.zeros((len(cases), 12), np.float32))
    worst = [0.0, 0.0]
    for s in (SCAN, GRID):
        batch = _call(eng, names, s)
        for i, name in enumerate(names):
            _check(name, batch, i, worst)
            assert _same(batch, _call(eng, [name], s), i, 0), (name, s)
        rows = _call(eng, names, s, rows=np.arange(len(names)))
        assert all(_same(batch, rows, i, i) for i in range(len(names))), s
        # rows in another order, one of them twice: the correspondences follow `rows`
        pick = [7, 3, 29, 7, 17, 5]
        sub = _call(eng, [names[i] for i in pick], s, rows=pick)
        assert all(_same(sub, batch, k, i) for k, i in enumerate(pick)), s
    print("batch of %d: worst rmse gap %.3g relative, worst information gap %.3g of the largest diagonal entry" % (len(names), worst[0], worst[1]))


def test_errors_are_found_before_anything_runs(eng):
    c = _cases()["size_257_5"]
    eng.set_option("icp_search", SCAN)   # (a fresh engine's default, compared with below)
    good = lambda **kw: eng.evaluate_registration([c["src"]], [c["dst"]], [c["T"]], want_information=True, want_correspondences=True, **kw)
    before = good(threshold=0.1)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(alignnet3d.EngineError, match="threshold"):
            good(threshold=bad)
    with pytest.raises(alignnet3d.EngineError, match="B < 1"):
        eng.evaluate_registration([], [], np.zeros((0, 4, 4)))
    fresh = alignnet3d.Engine(small_cfg(N=64, nb=12))
    with pytest.raises(alignnet3d.EngineError, match="no dataset"):
        fresh.evaluate_registration_rows([0], [np.eye(4)])
    fresh.upload_dataset(c["src"], c["dst"], np.array([[0, 0], [len(c["src"]), len(c["dst"])]]), np.zeros((1, 12), np.float32))
    for rows in ([1], [-1]):
        with pytest.raises(alignnet3d.EngineError, match="out of range"):
            fresh.evaluate_registration_rows(rows, [np.eye(4)])
    with pytest.raises(alignnet3d.EngineError, match="B < 1"):
        fresh.evaluate_registration_rows([], np.zeros((0, 4, 4)))
    assert _same(fresh.evaluate_registration_rows([0], [c["T"]], threshold=0.1, want_information=True, want_correspondences=True), before)
    fresh.close()
    assert _same(good(threshold=0.1), before)


def test_train_py_with_and_without_reg_eval(gpu_required, tmp_path):
    from tests.test_dropin_gpu import _make_dataset, _run
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import evaluation
    root = tmp_path / "SynthTiny"
    _make_dataset(str(root))
    # one epoch on 16 pairs predicts nothing: translations of 100 to 200 m came out.  The threshold is wide enough for such transforms to have inliers,
    # so that the numbers compared below are distances that depend on the transforms, the clouds and the rows, not zeros
    threshold = 500.0
    user = {"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
            "model": {"num_points": 64, "angles": {"num_bins": 12, "accept_inverted_angle": True},
                      "options": {"s1transformer": [[32, 64, 96], [[64, 32], 0.7]], "s2transformer": [[32, 64, 128], [[64, 32], 0.7]],
                                  "embedding": [32, 64, 160], "remaining_transform_prediction": [[64, 32], 0.7]}},
            "training": {"batch_size": 8, "num_epochs": 1, "learning_rate": 0.002},
            "evaluation": {"reg_eval": {"threshold": threshold}}}
    cfgp = tmp_path / "RegEval.json"
    json.dump(user, open(cfgp, "w"))
    out = _run(["train", "--config", str(cfgp)], str(tmp_path))
    ev = tmp_path / "logs" / "RegEval" / "val" / "eval000000"
    assert "Fitness: " in out and "Inlier RMSE: " in out
    val = list(range(16, 24))
    pred = {k: np.load(ev / (k + ".npy")) for k in ("pred_translations", "pred_angles", "pred_s2_pc1centers")}
    refs = []
    for i, vi in enumerate(val):
        T = evaluation.get_mat_angle(pred["pred_translations"][i], pred["pred_angles"][i], rotation_center=pred["pred_s2_pc1centers"][i])
        refs.append(R.evaluate_registration(np.load(root / "pointcloud1" / ("%08d.npy" % vi)), np.load(root / "pointcloud2" / ("%08d.npy" % vi)), T, threshold))
    assert sum(int(r["undecided"].sum()) for r in refs) <= R.POINT_CAP * sum(len(r["undecided"]) for r in refs)
    fit, rmse = np.load(ev / "reg_fitness.npy"), np.load(ev / "reg_inlier_rmse.npy")
    want_fit, want_rmse = np.array([r["fitness"] for r in refs]), np.array([r["rmse"] for r in refs])
    print("drop-in: fitness per pair", fit, "inlier rmse per pair", rmse, "predicted |translation|", np.linalg.norm(pred["pred_translations"], axis=1),
          "nearest distance per pair", [float(np.sqrt(r["dist2"].min())) for r in refs])
    assert np.array_equal(fit, want_fit) and np.allclose(rmse, want_rmse, rtol=RMSE_BAR, atol=0.0)
    for name in ("eval.json", "eval_180.json"):
        q = json.load(open(ev / name))["reg_eval"]
        assert abs(q["fitness"] - want_fit.mean()) <= 1e-15 and abs(q["inlier_rmse"] - want_rmse.mean()) <= RMSE_BAR * want_rmse.mean()
    assert want_fit.mean() > 0.0   # (the threshold is wide enough for this test to see inliers)
    # without the key: the reference's zeros, no array files, no quality fields in the log
    del user["evaluation"]
    json.dump(user, open(cfgp, "w"))
    out = _run(["eval_only", "--config", str(cfgp), "--eval_epoch", "0"], str(tmp_path))
    assert "Fitness: " not in out
    assert json.load(open(ev / "eval.json"))["reg_eval"] == {"fitness": 0.0, "inlier_rmse": 0.0}
    assert not (ev / "reg_fitness.npy").exists() and not (ev / "reg_inlier_rmse.npy").exists()
