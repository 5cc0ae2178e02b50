"""GPU: fast global registration (alignnet_fgr_register*, the fgr_* kernels of csrc/alignnet_globalreg.hip: the reference's o3_gicp_fast
baseline) against the fp64 restatement tests/fgr_ref.py, step by step, and the icp_global_fast.py command end to end.

Pinned-oracle method, as tests/test_global_reg_gpu.py: every step of the restatement is FED THE DEVICE'S OWN UPSTREAM OUTPUTS
(alignnet_debug_fgr_stages), so one flipped decision cannot cascade.  A reverse match whose margin is below G.UNDECIDED is undecided and
skipped, at most G.SKIP_CAP of them; a pair whose smallest tuple-test or score margin is below G.UNDECIDED_RANSAC is undecided, at most one of
the 8 pairs per estimate form (tests/test_fgr_cpu.py asserts that on these inputs the restatement alone finds a tenth of the first cap and no
undecided pair).  Transforms are held to 1e-9, the bar of tests/test_global_reg_gpu.py and tests/test_icp_gpu.py.  Stages 1-5 (downsample
to the forward matches) are the kernels tests/test_global_reg_gpu.py checks; here the forward matches are compared like the reverse ones:
a match between EQUAL rows is decided, the lowest index of the equal rows wins (global_reg_ref.matches).  The tests from test_new_pairs on
run global_reg_ref's NEW_PAIRS (filled, cluttered and far clouds) and all kinds of clouds side by side in one batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from tests import fgr_ref as R
from tests import global_reg_ref as G
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
KEYS = ("transforms", "fitness", "rmse", "correspondences", "trials")


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


def _check_pair(dev, constrained, decrease_mu, seed, stream, skipped, ties=None, **opt):
    """One pair's stage outputs against the restatement's steps, each from the device's upstream outputs.  Adds (skipped, total) of the match
    entries to `skipped`, and to `ties` the number of matches checked as ties between equal rows; returns False when the pair is undecided (a
    tuple-test or score margin below G.UNDECIDED_RANSAC)."""
    mcd, its = opt.get("maximum_correspondence_distance", R.MAX_CORR_DIST), opt.get("iteration_number", R.ITERATIONS)
    sp, tp = dev["points"]
    for name, key, (fa, fb) in (("matches", "matches", (0, 1)), ("reverse matches", "reverse_matches", (1, 0))):
        m, mm, tied = G.matches(dev["fpfh"][fa], dev["fpfh"][fb], with_ties=True)
        und = mm < G.UNDECIDED
        s = skipped.setdefault(name, [0, 0]); s[0] += int(und.sum()); s[1] += und.size
        assert np.array_equal(dev[key][~und], m[~und]), name
        if ties is not None:
            ties[name] = ties.get(name, 0) + int((tied & ~und).sum())
    cross = R.cross_check(dev["matches"], dev["reverse_matches"])
    assert np.array_equal(dev["cross"], cross)
    means, scale = R.normalise(sp, tp)
    np.testing.assert_allclose(dev["means"], means, rtol=1e-12, atol=0)
    np.testing.assert_allclose(dev["scale"], scale, rtol=1e-12, atol=0)
    ns, nt = R.apply_normalisation(sp, tp, dev["means"], dev["scale"])
    tup = R.tuple_test(ns, nt, dev["matches"], dev["cross"], seed, stream, opt.get("tuple_scale", R.TUPLE_SCALE),
                       opt.get("maximum_tuple_count", R.MAX_TUPLES))
    decided = tup["margin"] >= G.UNDECIDED_RANSAC
    print("cross %d, tuples %d in %d trials, margin %.3g | device: %d tuples in %d trials" % (
        len(cross), len(tup["accepted"]), tup["trials"], tup["margin"], len(dev["tuple_trials"]), dev["trials"]))
    if decided:
        assert np.array_equal(dev["tuple_trials"], tup["accepted"]) and dev["trials"] == tup["trials"]
        assert np.array_equal(dev["tuple_source"], tup["ci"]) and np.array_equal(dev["tuple_target"], tup["cj"])
    assert dev["correspondences"] == len(dev["tuple_source"]) == 3 * len(dev["tuple_trials"])
    # every iteration from the device's previous transform, on the device's correspondences
    P, Q0 = ns[dev["tuple_source"]], nt[dev["tuple_target"]]
    mus = R.mu_schedule(its, decrease_mu, opt.get("division_factor", R.DIVISION_FACTOR), mcd)
    T, worst, pivot = np.eye(4), 0.0, np.inf
    assert dev["trace"].shape == (its, 4, 4)
    for k in range(its):
        if len(P) < R.MIN_CORRESPONDENCES:
            want = T
        else:
            want, _, ratio = R.gn_step(T, mus[k], P, Q0, constrained)
            assert want is not None, "iteration %d: singular for the restatement" % k
            pivot = min(pivot, ratio)
        worst = max(worst, float(np.abs(dev["trace"][k] - want).max()))
        np.testing.assert_allclose(dev["trace"][k], want, rtol=0, atol=1e-9, err_msg="iteration %d" % k)
        T = dev["trace"][k]
    final = R.denormalise(T, dev["means"], dev["scale"])
    np.testing.assert_allclose(dev["transform"], final, rtol=0, atol=1e-9)
    cnt, fit, rmse, smargin = R.score(sp, tp, dev["transform"], mcd)
    print("iterations: worst step difference %.3g, smallest pivot ratio %.3g; fitness %.4f rmse %.6f (margin %.3g) | device: %.4f %.6f" % (
        worst, pivot, fit, rmse, smargin, dev["fitness"], dev["rmse"]))
    if smargin >= G.UNDECIDED_RANSAC:
        assert dev["fitness"] == fit and abs(dev["rmse"] - rmse) < 1e-9
    else:
        decided = False
    return decided


@pytest.mark.parametrize("decrease_mu", [False, True])
@pytest.mark.parametrize("constrained", [True, False])
def test_steps_match_restatement(eng, constrained, decrease_mu):
    src, dst, truth = G.gpu_test_pairs(constrained)
    skipped, undecided = {}, 0
    for k in range(len(src)):
        dev = eng.debug_fgr_stages(src[k], dst[k], constrained=constrained, decrease_mu=decrease_mu, seed=3, stream=k)
        undecided += 0 if _check_pair(dev, constrained, decrease_mu, 3, k, skipped) else 1
        E = np.linalg.inv(truth[k]) @ dev["transform"]
        print("pair %d: fitness %.3f, yaw error %.4f" % (k, dev["fitness"], abs(np.arctan2(E[1, 0], E[0, 0]))))
    for stage, (s, n) in skipped.items():
        print("%s: %d of %d entries undecided" % (stage, s, n))
        assert s <= G.SKIP_CAP * n, stage
    assert undecided <= 1


def test_defaults_large_and_degenerate(eng):
    s, d, truth = G.default_pair()
    dev = eng.debug_fgr_stages(s, d, seed=0, stream=5)
    assert _check_pair(dev, True, False, 0, 5, {})
    s2, d2, _ = G.large_pair()
    dev = eng.debug_fgr_stages(s2, d2, seed=1, stream=9)
    assert dev["counts"][1] > 6314, dev["counts"]
    skipped = {}
    assert _check_pair(dev, True, False, 1, 9, skipped)
    for stage, (sk, n) in skipped.items():
        assert sk <= G.SKIP_CAP * n, stage
    # fewer than 10 correspondences (three accepted tuples = 9): the identity of the normalised frame = the translation between the means
    dev = eng.debug_fgr_stages(s, d, seed=0, stream=5, maximum_tuple_count=3)
    assert _check_pair(dev, True, False, 0, 5, {}, maximum_tuple_count=3)
    want = np.eye(4); want[:3, 3] = dev["means"][1] - dev["means"][0]
    assert dev["correspondences"] == 9 and np.array_equal(dev["trace"], np.tile(np.eye(4), (64, 1, 1)))
    np.testing.assert_allclose(dev["transform"], want, rtol=0, atol=1e-12)
    # four tuples: the loop runs; no tuples at all; no iterations
    dev = eng.debug_fgr_stages(s, d, seed=0, stream=5, maximum_tuple_count=4, constrained=False)
    assert dev["correspondences"] == 12 and _check_pair(dev, False, False, 0, 5, {}, maximum_tuple_count=4)
    dev = eng.debug_fgr_stages(s, d, seed=0, stream=5, maximum_tuple_count=0)
    assert (dev["correspondences"], dev["trials"]) == (0, 0) and _check_pair(dev, True, False, 0, 5, {}, maximum_tuple_count=0)
    dev = eng.debug_fgr_stages(s, d, seed=0, stream=5, iteration_number=0)
    assert dev["trace"].shape == (0, 4, 4) and _check_pair(dev, True, False, 0, 5, {}, iteration_number=0)
    # more tuples than the optimise kernel holds in LDS (1024): the correspondences are read from HBM every iteration
    for constrained in (True, False):
        dev = eng.debug_fgr_stages(s, d, seed=0, stream=5, maximum_tuple_count=1100, constrained=constrained)
        assert dev["correspondences"] == 3300 and _check_pair(dev, constrained, False, 0, 5, {}, maximum_tuple_count=1100)
    # other option values reach the kernels
    opt = dict(division_factor=2.0, maximum_correspondence_distance=0.05, iteration_number=9, tuple_scale=0.9, maximum_tuple_count=40)
    dev = eng.debug_fgr_stages(s, d, seed=0, stream=5, decrease_mu=True, constrained=False, **opt)
    assert _check_pair(dev, False, True, 0, 5, {}, **opt)
    # a cloud so small that nothing passes (3 points), and empty clouds
    empty = np.zeros((0, 3), np.float32)
    src, dst, _ = G.gpu_test_pairs(True)
    res = eng.fgr_register([empty, src[0], empty, src[0][:3]], [dst[0], empty, empty, dst[0]])
    for k in range(3):
        assert np.array_equal(res["transforms"][k], np.eye(4)) and res["fitness"][k] == 0.0 and res["rmse"][k] == 0.0
        assert res["correspondences"][k] == 0 and res["trials"][k] == 0
    dev = eng.debug_fgr_stages(src[0][:3], dst[0], stream=3)
    assert dev["correspondences"] < 10 and _check_pair(dev, True, False, 0, 3, {})
    assert np.array_equal(res["transforms"][3], dev["transform"])
    np.testing.assert_allclose(dev["transform"][:3, 3], dev["means"][1] - dev["means"][0], rtol=0, atol=1e-12)
    dev = eng.debug_fgr_stages(empty, dst[0])
    assert dev["correspondences"] == 0 and len(dev["cross"]) == 0 and np.array_equal(dev["transform"], np.eye(4))


@pytest.mark.parametrize("name", ["volume", "volume_full", "clutter", "far"])
def test_new_pairs(eng, name):
    """Filled boxes (both max_nn cuts, the candidate spill), the cluttered object (zero and one-neighbour feature rows: ties in the matches
    BOTH ways, and a 15 m cloud under the 0.025 m score grid) and the far frame, step by step."""
    s, d, truth = G.new_pair(name)
    constrained = name != "volume_full"
    dev = eng.debug_fgr_stages(s, d, constrained=constrained, seed=3, stream=0)
    skipped, ties = {}, {}
    assert _check_pair(dev, constrained, False, 3, 0, skipped, ties)
    for stage, (sk, n) in skipped.items():
        print("%s: %d of %d entries undecided, %d checked as ties" % (stage, sk, n, ties[stage]))
        assert sk <= G.SKIP_CAP * n, stage
    assert dev["correspondences"] >= R.MIN_CORRESPONDENCES
    if name == "clutter":
        assert min(ties.values()) >= 30
        assert G.grid_cells(dev["points"][1], R.MAX_CORR_DIST) > G.MAX_GRID_CELLS
    if name in ("clutter", "far"):
        E = np.linalg.inv(truth) @ dev["transform"]
        print("fitness %.3f, yaw error %.4f" % (dev["fitness"], abs(np.arctan2(E[1, 0], E[0, 0]))))
        assert dev["fitness"] > 0.9 and abs(np.arctan2(E[1, 0], E[0, 0])) < 0.02


def test_heterogeneous_batch(eng):
    """A 24,000-point volume, three points, the cluttered object, an empty cloud and a plain object in one call: the stage arrays are strided
    by the largest cloud while three pairs are tiny.  Every output of every pair is bit for bit what the pair gives alone and through the
    stage hook."""
    vs, vd, _ = G.volume_pair(True)
    cs, cd, _ = G.clutter_pair()
    src, dst, _ = G.gpu_test_pairs(True)
    empty = np.zeros((0, 3), np.float32)
    S, D = [vs, src[0][:3], cs, empty, src[1]], [vd, dst[0], cd, dst[1], dst[1]]
    streams = [0, 12, 0, 14, 15]
    batch = eng.fgr_register(S, D, streams=streams, seed=3)
    print("correspondences", batch["correspondences"], "trials", batch["trials"], "fitness", batch["fitness"])
    assert batch["correspondences"][0] >= R.MIN_CORRESPONDENCES and batch["correspondences"][2] == 3 * R.MAX_TUPLES
    assert batch["correspondences"][3] == 0 and batch["fitness"][3] == 0.0
    for i in range(5):
        alone = eng.fgr_register([S[i]], [D[i]], streams=[streams[i]], seed=3)
        dbg = eng.debug_fgr_stages(S[i], D[i], stream=streams[i], seed=3)
        for k in KEYS:
            assert np.array_equal(alone[k][0], batch[k][i]), (i, k)
        for k, kd in zip(KEYS, ("transform", "fitness", "rmse", "correspondences", "trials")):
            assert np.array_equal(dbg[kd], batch[k][i]), (i, k)


def test_arguments(eng):
    src, dst, _ = G.gpu_test_pairs(True)
    with pytest.raises(RuntimeError, match="stream id"):
        eng.fgr_register(src[:1], dst[:1], streams=[1 << 24])
    with pytest.raises(RuntimeError, match="iteration_number"):
        eng.fgr_register(src[:1], dst[:1], iteration_number=-1)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="tuple_scale"):
            eng.fgr_register(src[:1], dst[:1], tuple_scale=bad)
    with pytest.raises(RuntimeError, match="maximum_tuple_count"):
        eng.fgr_register(src[:1], dst[:1], maximum_tuple_count=-1)
    with pytest.raises(RuntimeError, match="division_factor"):
        eng.fgr_register(src[:1], dst[:1], division_factor=0.5)
    with pytest.raises(RuntimeError, match="maximum_correspondence_distance"):
        eng.fgr_register(src[:1], dst[:1], maximum_correspondence_distance=0.0)
    with pytest.raises(RuntimeError, match="not finite"):
        bad = src[0].copy(); bad[5, 1] = np.nan
        eng.fgr_register([bad], dst[:1])
    import ctypes as C
    lib = eng._lib
    off = np.array([[0, 0], [len(src[0]), len(dst[0])]], np.int64)
    out = np.empty(16)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    call = lambda flags: lib.alignnet_fgr_register(eng._h, fp(src[0]), fp(dst[0]), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, flags, 0, None, 1.4, 0.025,
                                                   64, 0.95, 1000, out.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None)
    assert call(4) != 0 and b"unknown flags" in lib.alignnet_last_error(eng._h)
    assert call(0) == 0                                                                     # NULL streams = stream 0, NULL outputs
    assert np.array_equal(out.reshape(4, 4), eng.fgr_register(src[:1], dst[:1])["transforms"][0])
    assert call(2) == 0
    assert np.array_equal(out.reshape(4, 4), eng.fgr_register(src[:1], dst[:1], decrease_mu=True)["transforms"][0])


def test_result_depends_on_seed_stream_and_clouds_only(eng):
    src, dst, _ = G.gpu_test_pairs(True)
    src, dst = src[:4], dst[:4]
    streams = [40, 41, 42, 43]
    batch = eng.fgr_register(src, dst, streams=streams, seed=7)
    order = [2, 0, 3, 1]
    shuffled = eng.fgr_register([src[i] for i in order], [dst[i] for i in order], streams=[streams[i] for i in order], seed=7)
    off = np.zeros((5, 2), np.int64)
    off[1:, 0] = np.cumsum([len(x) for x in src]); off[1:, 1] = np.cumsum([len(x) for x in dst])
    eng.upload_dataset(np.concatenate(src), np.concatenate(dst), off, np.zeros((4, 12), np.float32))
    rows = eng.fgr_register_rows(order, streams=[streams[i] for i in order], seed=7)
    for k in KEYS:
        for pos, i in enumerate(order):
            assert np.array_equal(shuffled[k][pos], batch[k][i]) and np.array_equal(rows[k][pos], batch[k][i]), k
    for i in range(4):
        alone = eng.fgr_register([src[i]], [dst[i]], streams=[streams[i]], seed=7)
        dbg = eng.debug_fgr_stages(src[i], dst[i], stream=streams[i], seed=7)
        for k in KEYS:
            assert np.array_equal(alone[k][0], batch[k][i]), k
        assert np.array_equal(dbg["transform"], batch["transforms"][i]) and dbg["trials"] == batch["trials"][i]
    # default streams: the rows / 0 .. B - 1
    a = eng.fgr_register_rows([0, 1], seed=7)
    b = eng.fgr_register(src[:2], dst[:2], seed=7)
    for k in KEYS:
        assert np.array_equal(a[k], b[k])
    # another seed, another stream: other draws
    base = eng.debug_fgr_stages(src[0], dst[0], stream=40, seed=7)
    for kw in (dict(stream=40, seed=8), dict(stream=41, seed=7)):
        other = eng.debug_fgr_stages(src[0], dst[0], **kw)
        assert not np.array_equal(other["tuple_trials"], base["tuple_trials"]) and not np.array_equal(other["transform"], base["transform"])


def test_ransac_results_undisturbed_by_fgr(eng):
    src, dst, _ = G.gpu_test_pairs(True)
    kw = dict(seed=3, streams=[0, 1, 2], max_iteration=G.TEST_ITERATIONS, max_validation=G.TEST_VALIDATIONS)
    before = eng.global_register(src[:3], dst[:3], **kw)
    eng.fgr_register(src[:5], dst[:5], seed=1)
    eng.debug_fgr_stages(*G.large_pair()[:2])
    after = eng.global_register(src[:3], dst[:3], **kw)
    for k in ("transforms", "fitness", "rmse", "iterations", "validations"):
        assert np.array_equal(before[k], after[k]), k


# ---- the command, then train.py's refine step from its files ------------------------------------------------------------------------
def _make_dataset(root, n=12, nval=4):
    src, dst, truth = G.car_pairs(n, seed=41, n_points=1800, scale=0.3, max_shift=0.3)
    for sub in ("meta", "pointcloud1", "pointcloud2", "split"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    txt = lambda v: "\n".join("%.18e" % x for x in np.ravel(v)) + "\n"
    for i in range(n):
        c1 = src[i].astype(np.float64).mean(0)
        meta = {"translation": txt(truth[i][:3, 3]), "rel_angle": float(np.arctan2(truth[i][1, 0], truth[i][0, 0])),
                "start_position": txt(c1), "end_position": txt(truth[i][:3, :3] @ c1 + truth[i][:3, 3]), "start_angle": 0.0, "end_angle": 0.0}
        json.dump(meta, open(os.path.join(root, "meta", "%08d.json" % i), "w"))
        np.save(os.path.join(root, "pointcloud1", "%08d.npy" % i), src[i])
        np.save(os.path.join(root, "pointcloud2", "%08d.npy" % i), dst[i])
    open(os.path.join(root, "split", "train.txt"), "w").write("\n".join(map(str, range(n - nval))) + "\n")
    open(os.path.join(root, "split", "val.txt"), "w").write("\n".join(map(str, range(n - nval, n))) + "\n")
    return src[n - nval:], dst[n - nval:], truth[n - nval:], list(range(n - nval, n))


def _run(script, args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    r = subprocess.run([sys.executable, os.path.join(PKG, script)] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def _cfg(tmp_path, root, name, icp):
    p = tmp_path / (name + ".json")
    json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
               "evaluation": {"special": {"mode": "icp", "icp": icp}}}, open(p, "w"))
    return str(p)


def test_icp_global_fast_command_then_refine(gpu_required, tmp_path):
    sys.path.insert(0, PKG)
    import evaluation as EV
    from tests import icp_full_ref as F
    root = tmp_path / "SynthCars"
    vsrc, vdst, truth, ids = _make_dataset(str(root))
    logs = tmp_path / "logs" / "icp_SynthCars"
    cfg_g = _cfg(tmp_path, root, "icp_SynthCars_o3_gicp_fast", {"variant": "o3_gicp_fast", "with_constraint": True})
    r = _run("icp_global_fast.py", ["--config", cfg_g, "--seed", "2"], str(tmp_path))
    assert "Fast global registration (o3_gicp_fast" in r.stderr
    ev = logs / "icp_SynthCars_o3_gicp_fast" / "val" / "eval000000"
    pt, pa, pc = (np.load(ev / (k + ".npy")) for k in ("pred_translations", "pred_angles", "pred_s1_pc1centers"))
    assert pt.shape == (4, 3) and pa.shape == (4, 1) and pc.shape == (4, 3) and pt.dtype == np.float32 and np.all(pc == 0)
    js = [json.load(open(ev / f)) for f in ("eval.json", "eval_180.json")]
    assert all(j["mean_time"] > 0 for j in js) and js[0]["num"] == 4
    # what it stored is the engine's result for (seed 2, stream = example id, decrease_mu False)
    eng = alignnet3d.Engine(small_cfg(N=64, nb=12))
    res = eng.fgr_register(vsrc, vdst, seed=2, streams=ids)
    eng.close()
    np.testing.assert_array_equal(pt, res["transforms"][:, :3, 3].astype(np.float32))
    np.testing.assert_array_equal(pa[:, 0], EV.rotvec_z(res["transforms"][:, :3, :3]).astype(np.float32))
    # --use_old_results re-evaluates without registering; mean_time is kept
    before = [open(ev / f).read() for f in ("eval.json", "eval_180.json")]
    r = _run("icp_global_fast.py", ["--config", cfg_g, "--use_old_results"], str(tmp_path))
    assert "re-evaluated" in r.stderr and "Fast global registration (o3_gicp_fast" not in r.stderr
    assert [open(ev / f).read() for f in ("eval.json", "eval_180.json")] == before
    # train.py's refine step runs unchanged from those files, its mean_time on top of the stored one
    cfg_r = _cfg(tmp_path, root, "icp_SynthCars_o3_gicp_fast_p2p", {"variant": "o3_gicp_fast", "with_constraint": True, "refine": "p2p"})
    _run("train.py", ["train", "--config", cfg_r], str(tmp_path))
    ev2 = logs / "icp_SynthCars_o3_gicp_fast_p2p" / "val" / "eval000000"
    pt2, pa2 = np.load(ev2 / "pred_translations.npy"), np.load(ev2 / "pred_angles.npy")
    for k in range(4):
        init = EV.get_mat_angle(pt[k], pa[k], rotation_center=np.zeros(3))
        T = F.icp_p2point(vsrc[k], vdst[k], init, 0.10, 30, with_constraint=True)[0]
        np.testing.assert_allclose(pt2[k], T[:3, 3], rtol=0, atol=1e-6)
        np.testing.assert_allclose(pa2[k, 0], EV.rotvec_z(T[:3, :3]), rtol=0, atol=1e-6)
    assert json.load(open(ev2 / "eval_180.json"))["mean_time"] > js[1]["mean_time"]
    # a config it does not accept
    r = _run("icp_global_fast.py", ["--config", cfg_r], str(tmp_path), ok=False)
    assert r.returncode != 0 and "icp_global_fast.py accepts" in r.stderr
