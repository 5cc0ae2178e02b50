"""GPU: global registration (alignnet_global_register*, csrc/alignnet_globalreg.hip: FPFH + RANSAC, the reference's o3_gicp baseline)
against the fp64 restatement tests/global_reg_ref.py, stage by stage, and the icp_global.py command end to end.

Pinned-oracle method: every stage of the restatement is FED THE DEVICE'S OWN UPSTREAM OUTPUTS (alignnet_debug_global_stages), so one
flipped decision cannot cascade.  An entry whose decision margin (global_reg_ref's docstring) is below 1e-9 (1e-6 for the normals'
eigenvalue gap) is undecided and skipped; a stage may skip at most 1e-3 of its entries (tests/test_global_reg_cpu.py asserts that on these
inputs the restatement alone finds at most a tenth of that).  A RANSAC pair whose smallest comparison margin is below 1e-10 is undecided;
at most one of the 8 pairs per estimate form may be.  A match between EQUAL target rows is decided: the lowest index of the equal rows wins
(global_reg_ref.matches).

The thin surfaces of gpu_test_pairs / default_pair / large_pair never fill a neighbourhood; global_reg_ref's NEW_PAIRS do (the tests from
test_volume_pair on): both max_nn cuts and the candidate spill to HBM, isolated points, tied matches, a validation grid whose cell has to
grow, the voxel-span limit, a frame kilometres from the origin, and all of them side by side in one batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from tests import global_reg_ref as G
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
KEYS = ("transforms", "fitness", "rmse", "iterations", "validations")


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


def _check_front_end(dev, src, dst, skipped):
    """Stages 1-5 of one pair; adds (skipped, total) per stage to `skipped`.  Returns which matches were checked as ties between equal target
    rows (the lowest index of the equal rows is what they were compared with)."""
    def tally(stage, undecided):
        s = skipped.setdefault(stage, [0, 0])
        s[0] += int(undecided.sum()); s[1] += undecided.size
    for side, raw in enumerate((src, dst)):
        ds = G.voxel_downsample(raw)
        assert dev["counts"][side] == len(ds["points"])
        assert np.array_equal(dev["voxels"][side], ds["voxels"]) and np.array_equal(dev["voxel_points"][side], ds["counts"])
        P = dev["points"][side]
        np.testing.assert_allclose(P, ds["points"], rtol=1e-12, atol=0)
        nr = G.normals(P)
        und = (nr["nbr_margin"] < G.UNDECIDED) | (nr["gap"] < G.UNDECIDED_GAP) | (nr["nz"] < G.UNDECIDED)
        tally("normals", und)
        N = dev["normals"][side]
        np.testing.assert_allclose(N[~und], nr["normals"][~und], rtol=0, atol=1e-8)
        sp = G.spfh(P, N)
        und = (sp["nbr_margin"] < G.UNDECIDED) | (sp["margin"] < G.UNDECIDED)
        tally("spfh", und)
        S = dev["spfh"][side]
        np.testing.assert_allclose(S[~und], sp["spfh"][~und], rtol=0, atol=1e-7)
        fp = G.fpfh(P, S)
        und = fp["nbr_margin"] < G.UNDECIDED
        tally("fpfh", und)
        np.testing.assert_allclose(dev["fpfh"][side][~und], fp["fpfh"][~und], rtol=0, atol=1e-7)
    m, mm, tied = G.matches(dev["fpfh"][0], dev["fpfh"][1], with_ties=True)
    und = mm < G.UNDECIDED
    tally("matches", und)
    assert np.array_equal(dev["matches"][~und], m[~und])
    return tied & ~und


def _check_ransac(dev, constrained, seed, stream, max_iteration, max_validation):
    """RANSAC of one pair from the device's downsampled points and matches.  Returns False when the pair is undecided."""
    R = G.Ransac(dev["points"][0], dev["points"][1], dev["matches"], constrained, seed, stream)
    ref = R.run(max_iteration, max_validation)
    print("ransac: iterations %d validations %d win %d fitness %.4f rmse %.6f margin %.3g | device: %d %d %d %.4f %.6f"
          % (ref["iterations"], ref["validations"], ref["win"], ref["fitness"], ref["rmse"], ref["margin"],
             dev["iterations"], dev["validations"], dev["winning_iteration"], dev["fitness"], dev["rmse"]))
    if ref["margin"] < G.UNDECIDED_RANSAC:
        return False
    assert (dev["iterations"], dev["validations"]) == (ref["iterations"], ref["validations"])
    if dev["winning_iteration"] != ref["win"]:
        # a tie the restatement broke the other way: its own score of the device's winner must equal its best
        ok, T = R.prechecks(np.array([dev["winning_iteration"]]), track=False)
        assert ok[0]
        cnt, fit, rmse = R.score(T[0], track=False)
        assert fit == ref["fitness"] and abs(rmse - ref["rmse"]) < 1e-9
        np.testing.assert_allclose(dev["transform"], T[0], rtol=0, atol=1e-9)
    else:
        np.testing.assert_allclose(dev["transform"], ref["T"], rtol=0, atol=1e-9)
    assert dev["fitness"] == ref["fitness"] and abs(dev["rmse"] - ref["rmse"]) < 1e-9
    return True


@pytest.mark.parametrize("constrained", [True, False])
def test_stages_and_ransac_match_restatement(eng, constrained):
    src, dst, truth = G.gpu_test_pairs(constrained)
    skipped, undecided = {}, 0
    for k in range(len(src)):
        dev = eng.debug_global_stages(src[k], dst[k], constrained=constrained, seed=3, stream=k, max_iteration=G.TEST_ITERATIONS,
                                      max_validation=G.TEST_VALIDATIONS)
        _check_front_end(dev, src[k], dst[k], skipped)
        undecided += 0 if _check_ransac(dev, constrained, 3, k, G.TEST_ITERATIONS, G.TEST_VALIDATIONS) else 1
        assert dev["fitness"] > 0.9, "pair %d: the planted motion was not found" % k
    for stage, (s, n) in skipped.items():
        print("stage %s: %d of %d entries undecided" % (stage, s, n))
        assert s <= G.SKIP_CAP * n, stage
    assert undecided <= 1


def test_defaults_and_no_pass(eng):
    s, d, truth = G.default_pair()
    dev = eng.debug_global_stages(s, d, seed=0, stream=5)
    assert dev["validations"] == 500
    assert _check_ransac(dev, True, 0, 5, 4000000, 500)
    E = np.linalg.inv(truth) @ dev["transform"]
    assert dev["fitness"] > 0.95 and abs(np.arctan2(E[1, 0], E[0, 0])) < 0.02
    # so few iterations that no draw passes the checks: identity, fitness 0, every iteration run
    dev = eng.debug_global_stages(s, d, seed=0, stream=5, max_iteration=40, max_validation=500)
    ref = G.Ransac(dev["points"][0], dev["points"][1], dev["matches"], True, 0, 5).run(40, 500)
    assert ref["validations"] == 0
    assert (dev["iterations"], dev["validations"], dev["winning_iteration"], dev["fitness"], dev["rmse"]) == (40, 0, -1, 0.0, 0.0)
    assert np.array_equal(dev["transform"], np.eye(4))


def test_result_depends_on_seed_stream_and_clouds_only(eng):
    src, dst, _ = G.gpu_test_pairs(True)
    src, dst = src[:4], dst[:4]
    kw = dict(seed=7, max_iteration=G.TEST_ITERATIONS, max_validation=G.TEST_VALIDATIONS)
    streams = [40, 41, 42, 43]
    batch = eng.global_register(src, dst, streams=streams, **kw)
    order = [2, 0, 3, 1]
    shuffled = eng.global_register([src[i] for i in order], [dst[i] for i in order], streams=[streams[i] for i in order], **kw)
    off = np.zeros((5, 2), np.int64)
    off[1:, 0] = np.cumsum([len(x) for x in src]); off[1:, 1] = np.cumsum([len(x) for x in dst])
    eng.upload_dataset(np.concatenate(src), np.concatenate(dst), off, np.zeros((4, 12), np.float32))
    rows = eng.global_register_rows(order, streams=[streams[i] for i in order], **kw)
    for k in KEYS:
        for pos, i in enumerate(order):
            assert np.array_equal(shuffled[k][pos], batch[k][i]) and np.array_equal(rows[k][pos], batch[k][i]), k
    for i in range(4):
        alone = eng.global_register([src[i]], [dst[i]], streams=[streams[i]], **kw)
        dbg = eng.debug_global_stages(src[i], dst[i], stream=streams[i], **kw)
        for k in KEYS:
            assert np.array_equal(alone[k][0], batch[k][i]), k
        assert np.array_equal(dbg["transform"], batch["transforms"][i]) and dbg["iterations"] == batch["iterations"][i]
    # default streams: the rows / 0 .. B - 1
    a = eng.global_register_rows([0, 1], **kw)
    b = eng.global_register(src[:2], dst[:2], **kw)
    for k in KEYS:
        assert np.array_equal(a[k], b[k])
    # another seed draws differently
    wins = [[eng.debug_global_stages(src[i], dst[i], stream=streams[i], seed=sd, max_iteration=G.TEST_ITERATIONS,
                                     max_validation=G.TEST_VALIDATIONS)["winning_iteration"] for i in range(2)] for sd in (7, 8)]
    assert wins[0] != wins[1]


def test_edge_cases(eng):
    src, dst, _ = G.gpu_test_pairs(True)
    empty = np.zeros((0, 3), np.float32)
    tiny = src[0][:3]
    one_voxel = (src[0][:1] + np.random.default_rng(0).uniform(0, 0.001, (50, 3))).astype(np.float32)
    kw = dict(max_iteration=20000, max_validation=20)
    res = eng.global_register([empty, src[0], tiny, one_voxel, empty], [dst[0], empty, dst[0], dst[0], empty], **kw)
    for k in range(5):
        assert np.array_equal(res["transforms"][k], np.eye(4)) and res["fitness"][k] == 0.0 and res["rmse"][k] == 0.0
        assert res["iterations"][k] == 0 and res["validations"][k] == 0
    # a target above the LDS-resident size (> 6314 downsampled points): the validation grid is read from HBM.  The same pair through
    # both paths of the restatement's decisions: stage by stage, as above
    s, d, truth = G.large_pair()
    dev = eng.debug_global_stages(s, d, seed=1, stream=9, max_iteration=100000, max_validation=20)
    assert dev["counts"][1] > 6314, dev["counts"]
    skipped = {}
    _check_front_end(dev, s, d, skipped)
    for stage, (sk, n) in skipped.items():
        assert sk <= G.SKIP_CAP * n, stage
    assert _check_ransac(dev, True, 1, 9, 100000, 20)
    # arguments
    with pytest.raises(RuntimeError, match="stream id"):
        eng.global_register(src[:1], dst[:1], streams=[1 << 24], **kw)
    with pytest.raises(RuntimeError, match="max_iteration"):
        eng.global_register(src[:1], dst[:1], max_iteration=(1 << 38) + 1)
    with pytest.raises(RuntimeError, match="not finite"):
        bad = src[0].copy(); bad[5, 1] = np.nan
        eng.global_register([bad], dst[:1], **kw)
    lib = eng._lib
    import ctypes as C
    off = np.array([[0, 0], [len(src[0]), len(dst[0])]], np.int64)
    out = np.empty(16)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.alignnet_global_register(eng._h, fp(src[0]), fp(dst[0]), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, 2, 0, None, 100, 5,
                                      out.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None)
    assert rc != 0 and b"unknown flags" in lib.alignnet_last_error(eng._h)
    rc = lib.alignnet_global_register(eng._h, fp(src[0]), fp(dst[0]), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, 0, 0, None, 20000, 5,
                                      out.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None)   # NULL streams = stream 0
    assert rc == 0
    assert np.array_equal(out.reshape(4, 4), eng.global_register(src[:1], dst[:1], max_iteration=20000, max_validation=5)["transforms"][0])


# ---- filled, cluttered, far and wide clouds (global_reg_ref.NEW_PAIRS; tests/test_global_reg_cpu.py holds what they reach and that the
# ---- restatement alone decides them) ---------------------------------------------------------------------------------------------------
def _report(skipped):
    for stage, (s, n) in skipped.items():
        print("stage %s: %d of %d entries undecided" % (stage, s, n))
        assert s <= G.SKIP_CAP * n, stage


@pytest.mark.parametrize("constrained", [True, False])
def test_volume_pair(eng, constrained):
    """Every neighbourhood of the features is cut to its 100 nearest, half of them after more than kCandLds candidates (ranked from HBM), and
    40 % of the normals' to their 30 nearest."""
    s, d, _ = G.volume_pair(constrained)
    dev = eng.debug_global_stages(s, d, constrained=constrained, seed=3, stream=0, max_iteration=G.VOLUME_ITERATIONS, max_validation=G.VOLUME_VALIDATIONS)
    for P in dev["points"]:
        c10, c25 = G.radius_counts(P, 2 * G.VOXEL), G.radius_counts(P, 5 * G.VOXEL)
        assert (c10 > 30).sum() >= 500 and (c25 > G.CAND_LDS).sum() >= 500 and c25.min() > 100
    skipped = {}
    _check_front_end(dev, s, d, skipped)
    _report(skipped)
    assert _check_ransac(dev, constrained, 3, 0, G.VOLUME_ITERATIONS, G.VOLUME_VALIDATIONS)
    assert dev["validations"] >= 1


def test_clutter_pair(eng):
    """Stray points around the object: default normals and all-zero feature rows where nothing is near, the one-neighbour histogram, matches
    tied between equal rows, and a 15 m cloud for the validation grid (9 million cells at the threshold's size; it holds 32,768)."""
    s, d, truth = G.clutter_pair()
    dev = eng.debug_global_stages(s, d, seed=3, stream=0, max_iteration=G.TEST_ITERATIONS, max_validation=G.TEST_VALIDATIONS)
    skipped = {}
    tied = _check_front_end(dev, s, d, skipped)
    _report(skipped)
    print("tied matches checked: %d of %d" % (tied.sum(), tied.size))
    assert tied.sum() >= 30
    for side in range(2):
        P = dev["points"][side]
        for radius, name in ((2 * G.VOXEL, "normals"), (5 * G.VOXEL, "fpfh")):
            assert (G.neighbours(P, radius, len(P) + 1)[4] >= G.UNDECIDED).all()      # every count below is decided
        c10, c25 = G.radius_counts(P, 2 * G.VOXEL), G.radius_counts(P, 5 * G.VOXEL)
        print("side %d: %d points with K < 3 at 0.10, %d with K < 2 and %d with K == 2 at 0.25" % (side, (c10 < 3).sum(), (c25 < 2).sum(), (c25 == 2).sum()))
        assert (c10 < 3).sum() >= 10 and (c25 < 2).sum() >= 10 and (c25 == 2).sum() >= 10
        assert np.array_equal(dev["normals"][side][c10 < 3], np.tile([0.0, 0.0, 1.0], ((c10 < 3).sum(), 1)))
        for key in ("spfh", "fpfh"):
            F = dev[key][side]
            assert not F[c25 < 2].any() and (np.abs(F[c25 >= 2]).sum(1) > 0).all(), key
        # one neighbour: three bins of exactly 100 / (K - 1) = 100
        assert np.array_equal(np.sort(dev["spfh"][side][c25 == 2], 1)[:, -4:], np.tile([0.0, 100.0, 100.0, 100.0], ((c25 == 2).sum(), 1)))
    assert G.grid_cells(dev["points"][1]) > G.MAX_GRID_CELLS
    assert _check_ransac(dev, True, 3, 0, G.TEST_ITERATIONS, G.TEST_VALIDATIONS)
    E = np.linalg.inv(truth) @ dev["transform"]
    assert dev["fitness"] > 0.9 and abs(np.arctan2(E[1, 0], E[0, 0])) < 0.02


def test_far_pair(eng):
    """4 km from the origin float32 coordinates are 2.4e-4 m apart and raw points sit on voxel edges up to the rounding of 0.05 and 0.025: the
    voxels and their counts are compared exactly (an fp32 floor, or a reciprocal in place of the division, puts those points elsewhere)."""
    s, d, truth = G.far_pair()
    dev = eng.debug_global_stages(s, d, seed=3, stream=0, max_iteration=G.TEST_ITERATIONS, max_validation=G.TEST_VALIDATIONS)
    edge = 0
    for side, raw in enumerate((s, d)):
        ds = G.voxel_downsample(raw)
        edge += int((ds["margin"] < 1e-9).sum())
        assert ds["margin"].min() > 1e-13
        assert dev["counts"][side] == len(ds["points"])
        assert np.array_equal(dev["voxels"][side], ds["voxels"]) and np.array_equal(dev["voxel_points"][side], ds["counts"])
    print("raw points within 1e-9 bin widths of a voxel edge: %d" % edge)
    assert edge >= 1
    skipped = {}
    _check_front_end(dev, s, d, skipped)
    _report(skipped)
    assert _check_ransac(dev, True, 3, 0, G.TEST_ITERATIONS, G.TEST_VALIDATIONS)
    E = np.linalg.inv(truth) @ dev["transform"]
    assert dev["fitness"] > 0.9 and abs(np.arctan2(E[1, 0], E[0, 0])) < 0.02


def test_wide_pair_and_span_limit(eng):
    """One point 100,000 m away: 2,000,000 voxels, inside the limit, and a validation grid whose cell grows from 0.075 m to metres.  Two
    points 110,000 m apart are more than 2^21 voxels: refused, and the engine computes afterwards what it computed before."""
    s, d, _ = G.wide_pair()
    kw = dict(seed=3, stream=0, max_iteration=G.WIDE_ITERATIONS, max_validation=G.WIDE_VALIDATIONS)
    dev = eng.debug_global_stages(s, d, **kw)
    assert dev["voxels"][1][:, 0].max() >= 2000000 and G.grid_cells(dev["points"][1]) > G.MAX_GRID_CELLS
    skipped = {}
    _check_front_end(dev, s, d, skipped)
    _report(skipped)
    assert _check_ransac(dev, True, 3, 0, G.WIDE_ITERATIONS, G.WIDE_VALIDATIONS)
    assert dev["validations"] == G.WIDE_VALIDATIONS
    src, dst, _ = G.gpu_test_pairs(True)
    batch = dict(seed=3, streams=[0, 7], max_iteration=G.WIDE_ITERATIONS, max_validation=G.WIDE_VALIDATIONS)
    before = eng.global_register([s, src[0]], [d, dst[0]], **batch)
    wide = G.too_wide_cloud()
    for a, b in ((wide, dst[0]), (src[0], wide)):
        with pytest.raises(RuntimeError, match=r"2\^21 voxels"):
            eng.global_register([src[1], a], [dst[1], b], **batch)
        with pytest.raises(RuntimeError, match=r"2\^21 voxels"):
            eng.debug_global_stages(a, b, **kw)
    after = eng.global_register([s, src[0]], [d, dst[0]], **batch)
    for k in KEYS:
        assert np.array_equal(before[k], after[k]), k
    again = eng.debug_global_stages(s, d, **kw)
    for k in ("transform", "matches"):
        assert np.array_equal(again[k], dev[k]), k
    for k in ("points", "normals", "spfh", "fpfh"):
        assert all(np.array_equal(x, y) for x, y in zip(again[k], dev[k])), k


def test_heterogeneous_batch(eng):
    """A 24,000-point volume, three points, the cluttered object, an empty cloud and a plain object in one call: the stage arrays are strided
    by the largest cloud while three pairs are tiny.  Every output of every pair is bit for bit what the pair gives alone and through the
    stage hook."""
    vs, vd, _ = G.volume_pair(True)
    cs, cd, _ = G.clutter_pair()
    src, dst, _ = G.gpu_test_pairs(True)
    empty = np.zeros((0, 3), np.float32)
    S, D = [vs, src[0][:3], cs, empty, src[1]], [vd, dst[0], cd, dst[1], dst[1]]
    streams = [0, 12, 0, 14, 15]            # the volume and the clutter pair as their own tests draw them: validations are known to be reached
    kw = dict(seed=3, max_iteration=G.VOLUME_ITERATIONS, max_validation=G.VOLUME_VALIDATIONS)
    batch = eng.global_register(S, D, streams=streams, **kw)
    print("validations", batch["validations"], "fitness", batch["fitness"])
    assert batch["validations"][0] >= 1 and batch["validations"][2] == G.VOLUME_VALIDATIONS
    assert batch["fitness"][1] == 0.0 and batch["fitness"][3] == 0.0
    for i in range(5):
        alone = eng.global_register([S[i]], [D[i]], streams=[streams[i]], **kw)
        dbg = eng.debug_global_stages(S[i], D[i], stream=streams[i], **kw)
        for k in KEYS:
            assert np.array_equal(alone[k][0], batch[k][i]), (i, k)
        for k, kd in zip(KEYS, ("transform", "fitness", "rmse", "iterations", "validations")):
            assert np.array_equal(dbg[kd], batch[k][i]), (i, k)


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


def test_icp_global_command_then_refine(gpu_required, tmp_path):
    sys.path.insert(0, PKG)
    import evaluation as EV
    from tests import icp_full_ref as F
    root = tmp_path / "SynthCars"
    vsrc, vdst, truth, ids = _make_dataset(str(root))
    logs = tmp_path / "logs" / "icp_SynthCars"
    cfg_g = _cfg(tmp_path, root, "icp_SynthCars_o3_gicp", {"variant": "o3_gicp", "with_constraint": True})
    r = _run("icp_global.py", ["--config", cfg_g, "--seed", "2"], str(tmp_path))
    assert "Global registration (o3_gicp" in r.stderr
    ev = logs / "icp_SynthCars_o3_gicp" / "val" / "eval000000"
    pt, pa, pc = (np.load(ev / (k + ".npy")) for k in ("pred_translations", "pred_angles", "pred_s1_pc1centers"))
    assert pt.shape == (4, 3) and pa.shape == (4, 1) and pc.shape == (4, 3) and pt.dtype == np.float32 and np.all(pc == 0)
    js = [json.load(open(ev / f)) for f in ("eval.json", "eval_180.json")]
    assert all(j["mean_time"] > 0 for j in js) and js[0]["num"] == 4
    # what it stored is the engine's result for (seed 2, stream = example id)
    eng = alignnet3d.Engine(small_cfg(N=64, nb=12))
    res = eng.global_register(vsrc, vdst, seed=2, streams=ids)
    eng.close()
    np.testing.assert_array_equal(pt, res["transforms"][:, :3, 3].astype(np.float32))
    np.testing.assert_array_equal(pa[:, 0], EV.rotvec_z(res["transforms"][:, :3, :3]).astype(np.float32))
    for k in range(4):
        E = np.linalg.inv(truth[k]) @ res["transforms"][k]
        assert abs(np.arctan2(E[1, 0], E[0, 0])) < 0.03, (k, E)
    # --use_old_results re-evaluates without registering; mean_time is kept
    before = [open(ev / f).read() for f in ("eval.json", "eval_180.json")]
    r = _run("icp_global.py", ["--config", cfg_g, "--use_old_results"], str(tmp_path))
    assert "re-evaluated" in r.stderr and "Global registration (o3_gicp" not in r.stderr
    assert [open(ev / f).read() for f in ("eval.json", "eval_180.json")] == before
    # train.py's refine step runs unchanged from those files, its mean_time on top of the stored one
    cfg_r = _cfg(tmp_path, root, "icp_SynthCars_o3_gicp_p2p", {"variant": "o3_gicp", "with_constraint": True, "refine": "p2p"})
    _run("train.py", ["train", "--config", cfg_r], str(tmp_path))
    ev2 = logs / "icp_SynthCars_o3_gicp_p2p" / "val" / "eval000000"
    pt2, pa2 = np.load(ev2 / "pred_translations.npy"), np.load(ev2 / "pred_angles.npy")
    for k in range(4):
        init = EV.get_mat_angle(pt[k], pa[k], rotation_center=np.zeros(3))
        T = F.icp_p2point(vsrc[k], vdst[k], init, 0.10, 30, with_constraint=True)[0]
        np.testing.assert_allclose(pt2[k], T[:3, 3], rtol=0, atol=1e-6)
        np.testing.assert_allclose(pa2[k, 0], EV.rotvec_z(T[:3, :3]), rtol=0, atol=1e-6)
    assert json.load(open(ev2 / "eval_180.json"))["mean_time"] > js[1]["mean_time"]
    # a config it does not accept
    r = _run("icp_global.py", ["--config", cfg_r], str(tmp_path), ok=False)
    assert r.returncode != 0 and "icp_global.py accepts" in r.stderr
