"""GPU: generalized ICP (Engine.icp_generalized_refine*, csrc/alignnet_icp.hip: the normals kernels on both clouds, icp_surface_kernel<true, .>) against
the fp64 restatement tests/icp_generalized_ref.py.  Stage by stage through Engine.debug_icp_generalized (the shipped source compiled with a record
behind it), every stage fed the DEVICE's own upstream outputs: both clouds' neighbour counts equal, normals to 1e-8, index / inlier / fitness equal,
squared distances to 1e-12 relative, every sum within 64 n u sum |term| (n = the inliers, u = 2^-53: the terms are the restatement's to the bit, the
order of summation is not; tests/icp_generalized_ref.py derives the bound), the update within 1e-9 of the restatement's solve of the device's sums.
Whole runs to the bars of tests/test_icp_plane_gpu.py: transforms within 1e-9 max(1, |offset|), rmse within 1e-9, fitness and iteration counts
equal.  An entry within the margins of a decision (P.UNDECIDED, P.UNDECIDED_GAP) is left out of its stage's comparison; at most P.SKIP_CAP of a
stage's entries may be."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import alignnet3d
from tests import icp_generalized_ref as G
from tests import icp_plane_ref as P
from tests.helpers import small_cfg, oracle_params
from tests.test_icp_plane_gpu import _make_dataset, _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
RADIUS, NORMAL_RADIUS = 0.1, 0.3
KEYS = ("transforms", "fitness", "rmse", "iterations")


def _engine():
    return alignnet3d.Engine(small_cfg(N=64, nb=12))


def _check_normals(name, which, pts, got_n, got_k, normal_radius, tally):
    nr = P.normals(pts, normal_radius)
    und = P.normals_undecided(nr)
    tally[0] += int(und.sum()); tally[1] += len(pts)
    sure = nr["nbr_margin"] >= P.UNDECIDED
    assert np.array_equal(got_k[sure], nr["count"][sure]), (name, which, "neighbour counts")
    nerr = np.abs(got_n - nr["normals"]).max(1) if len(pts) else np.zeros(0)
    print("%s %s: %d points, neighbours mean %.1f max %d, normals undecided %d, worst normal error %.3g"
          % (name, which, len(pts), got_k.mean() if len(pts) else 0, got_k.max() if len(pts) else 0, und.sum(), nerr[~und].max() if (~und).any() else 0.0))
    assert np.all(nerr[~und] <= 1e-8), (name, which, "normals")
    few = got_k < 3
    assert np.all(got_n[:, 2] >= 0) and np.array_equal(got_n[few], np.tile([0.0, 0.0, 1.0], (int(few.sum()), 1))), (name, which)


def _stages(eng, name, src, dst, T, tally, radius=RADIUS, normal_radius=NORMAL_RADIUS):
    """One pair through the read-back, both estimates.  tally: [normals skipped, normals, points skipped, points]."""
    dst64 = np.asarray(dst, np.float64).reshape(-1, 3)
    e = P.evaluate(src, dst, T, radius) if len(dst) and len(src) else None
    out = {}
    for constrained in (True, False):
        full = not constrained
        d = eng.debug_icp_generalized(src, dst, T, radius=radius, normal_radius=normal_radius, constrained=constrained)
        out[constrained] = d
        # 1. normals of both clouds
        t0 = tally if constrained else [0, 0]
        _check_normals(name, "target", dst, d["normals"], d["neighbours"], normal_radius, t0)
        _check_normals(name, "source", src, d["source_normals"], d["source_neighbours"], normal_radius, t0)
        if e is None:
            assert d["fitness"] == 0.0 and d["rmse"] == 0.0 and not d["inlier"].any() and np.all(d["index"] == -1) and np.array_equal(d["update"], np.eye(4))
            assert not d["sums"].any()
            continue
        # 2. the evaluation
        ok = ~e["undecided"]
        if constrained:
            tally[2] += int((~ok).sum()); tally[3] += len(src)
        inl = ok & e["inlier"]
        assert np.array_equal(d["inlier"][ok], e["inlier"][ok]), (name, "inliers")
        assert np.array_equal(d["index"][inl], e["index"][inl]), (name, "index")
        if ok.all():
            assert d["fitness"] == e["fitness"], (name, d["fitness"], e["fitness"])
        rel = np.abs(d["dist2"][inl] - e["best"][inl]) / np.maximum(e["best"][inl], 1e-300)
        assert np.all(d["dist2"][inl] == e["best"][inl]) or rel.max() <= 1e-12, (name, "dist2", rel.max())
        # 3. the sums, of the device's correspondences, normals (both clouds') and distances
        di = d["inlier"]
        j = d["index"][di]
        c = dst64[0]
        s, mag, n = G.sums(e["p"][di], dst64[j], d["normals"][j], d["source_normals"][di], T, d["dist2"][di], c, full)
        bound = 64.0 * n * G.U64 * mag
        worst = (np.abs(d["sums"] - s) / np.maximum(n * G.U64 * mag, 1e-300)).max()
        print("%s constrained %d: fitness %.4f, %d undecided points, worst relative dist2 error %.3g, worst sum error %.3g n u sum |term| (bar 64)"
              % (name, constrained, d["fitness"], (~ok).sum(), rel.max() if rel.size else 0, worst))
        assert d["sums"][0] == n and np.all(np.abs(d["sums"] - s) <= bound), (name, "sums", np.abs(d["sums"] - s), bound)
        assert not d["sums"][G.nsums(full):].any()
        assert abs(d["rmse"] - (np.sqrt(d["sums"][1] / n) if n else 0.0)) <= 1e-15
        # 4. the update, from the device's sums
        info = {}
        U, det = P.solve(d["sums"], c, full, info)
        print("   update: determined %d, scaled condition number %.3g, error %.3g" % (det, info["cond"], np.abs(d["update"] - U).max()))
        assert det or np.array_equal(d["update"], np.eye(4)), (name, "an undetermined update is the identity")
        assert not det or info["cond"] <= 1e4, (name, "the inputs are to be well conditioned", info["cond"])
        np.testing.assert_allclose(d["update"], U, rtol=0, atol=1e-9, err_msg=name)
    return out


def _capped(tally):
    return tally[0] <= P.SKIP_CAP * tally[1] and tally[2] <= P.SKIP_CAP * tally[3]


@functools.lru_cache(maxsize=None)
def _car():
    src, dst, truth = P.car_pair(10.0, 1, scale=4.4)
    return src, dst, P.disturbed(truth, src.astype(np.float64).mean(0), seed=1)


# ---- 1. stage parity ------------------------------------------------------------------------------------------------------------------------------
def test_stages_corner_car_and_far_frame(gpu_required):
    eng = _engine()
    tally = [0, 0, 0, 0]
    src, dst, init, _ = P.corner_pair(900, 1, constrained=False)
    d = _stages(eng, "corner 900", src, dst, init, tally)
    assert d[True]["fitness"] > 0.5
    src, dst, init = _car()
    _stages(eng, "car scan", src, dst, init, tally)
    src, dst, init, _ = P.corner_pair(2000, 2, offset=5000.0, constrained=False, side=2.5)   # 5 km out: float32 coordinates on a 0.5 mm lattice
    _stages(eng, "corner 5 km", src, dst, init, tally)
    assert _capped(tally), tally
    eng.close()


def test_stages_source_normal_edges(gpu_required):
    """Sources of 1, 2 and 3 points, 48 source points without neighbours, source sizes around one workgroup of the normals kernel (256 lanes), an empty
    source, an empty target.  (A source beyond 1024 workgroups x 256 lanes -- 262,145 points, where a lane takes a second point -- is left out: its
    restatement alone takes longer than this file; the stride is the loop the target's kernel runs in tests/test_icp_plane_gpu.py.)"""
    eng = _engine()
    tally = [0, 0, 0, 0]
    src, dst, init, _ = P.corner_pair(600, 4)
    for n1 in (1, 2, 3, 255, 256, 257):
        d = _stages(eng, "n1 %d" % n1, src[:n1], dst, init, tally)[True]
        assert len(d["source_normals"]) == n1 == len(d["source_neighbours"]) and d["source_neighbours"].min() >= 1
    # 48 strays in the source, each alone in its neighbourhood and far from every target: K = 1, the default normal, no correspondence
    rng = np.random.default_rng(9)
    strays = (src.astype(np.float64).mean(0) + np.stack([4.0 + 0.7 * np.arange(48), rng.uniform(-1, 1, 48), rng.uniform(-1, 1, 48)], 1)).astype(np.float32)
    mixed = np.concatenate([src[:100], strays, src[100:]])
    d = _stages(eng, "48 strays", mixed, dst, init, tally)[True]
    assert np.all(d["source_neighbours"][100:148] == 1) and not d["inlier"][100:148].any()
    assert np.array_equal(d["source_normals"][100:148], np.tile([0.0, 0.0, 1.0], (48, 1)))
    # strays that DO land on targets: the default source normal enters the weights
    inv = np.linalg.inv(init)
    near = ((dst[:6].astype(np.float64) + [0.01, -0.02, 0.015]) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    _stages(eng, "6 points alone", near[::2], dst, init, tally)
    _stages(eng, "empty source", src[:0], dst, init, tally)
    _stages(eng, "empty target", src[:40], dst[:0], init, tally)
    for n2 in (1, 2, 3):
        _stages(eng, "n2 %d" % n2, src[:40], dst[:n2], init, tally)
    assert _capped(tally), tally
    eng.close()


@pytest.mark.parametrize("tilt", [(0.0, 0.0), (0.25, -0.125)])
def test_single_plane_moves_by_the_planted_shift(gpu_required, tilt):
    eng = _engine()
    src, dst = P.plane_pair(600, 4, tilt)
    tally = [0, 0, 0, 0]
    d = _stages(eng, "plane %s" % (tilt,), src, dst, np.eye(4), tally)
    planted = P.rigid_about(np.zeros(3), (0.0, 0.0, 0.0), np.array([0.0, 0.0, -0.03]))
    for constrained in (True, False):
        assert not np.array_equal(d[constrained]["update"], np.eye(4)) and d[constrained]["fitness"] > 0.9
        ref = G.icp_generalized(src, dst, np.eye(4), RADIUS, NORMAL_RADIUS, 30, constrained)
        res = eng.icp_generalized_refine([src], [dst], [np.eye(4)], constrained=constrained)
        print("tilt %s constrained %d: %d iterations, device - restatement %.3g, device - planted %.3g"
              % (tilt, constrained, res["iterations"][0], np.abs(res["transforms"][0] - ref[0]).max(), np.abs(res["transforms"][0] - planted).max()))
        # (duplicate grid points of the plane tie exactly: the lowest index wins on both sides, so the run is compared whatever ref[4] counts)
        np.testing.assert_allclose(res["transforms"][0], ref[0], rtol=0, atol=1e-9)
        assert res["iterations"][0] == ref[3] <= 5 and res["fitness"][0] == ref[1] and abs(res["rmse"][0] - ref[2]) < 1e-9
        assert np.abs(res["transforms"][0] - planted).max() <= 1e-6
        same = eng.icp_plane_refine([src], [dst], [np.eye(4)], constrained=constrained)          # point-to-plane determines nothing here
        assert np.array_equal(same["transforms"][0], np.eye(4))
    eng.close()


# ---- 2. whole runs ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_reference(constrained):
    srcs, dsts, inits = G.batch_pairs()
    return [G.icp_generalized(s, d, i, RADIUS, NORMAL_RADIUS, 30, constrained) for s, d, i in zip(srcs, dsts, inits)]


def test_whole_runs_batch_alone_and_dataset(gpu_required):
    eng = _engine()
    srcs, dsts, inits = G.batch_pairs()
    B = len(srcs)
    off = np.zeros((B + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(s) for s in srcs]); off[1:, 1] = np.cumsum([len(t) for t in dsts])
    eng.upload_dataset(np.concatenate(srcs), np.concatenate(dsts), off, np.zeros((B, 12), np.float32))
    kw = dict(radius=RADIUS, normal_radius=NORMAL_RADIUS, its=30)
    skipped = 0
    for constrained in (True, False):
        res = eng.icp_generalized_refine(srcs, dsts, inits, constrained=constrained, **kw)
        refs = _batch_reference(constrained)
        for k in range(B):
            T, fit, rmse, it, und = refs[k]
            scale = max(1.0, float(np.abs(dsts[k]).max()) if len(dsts[k]) else 1.0)
            err = np.abs(res["transforms"][k] - T).max()
            print("pair %d (n1 %d n2 %d) constrained %d: fitness %.4f, %d iterations (device %d), %d undecided, transform error %.3g (bar %.3g), rmse error %.3g"
                  % (k, len(srcs[k]), len(dsts[k]), constrained, fit, it, res["iterations"][k], und, err, 1e-9 * scale, abs(res["rmse"][k] - rmse)))
            if und:
                skipped += 1
                continue
            np.testing.assert_allclose(res["transforms"][k], T, rtol=0, atol=1e-9 * scale, err_msg="pair %d" % k)
            assert res["fitness"][k] == fit and res["iterations"][k] == it and abs(res["rmse"][k] - rmse) < 1e-9, k
        # every pair alone: bit-identical (the chunking, the shared workspace and the order inside a grid bucket leave no trace)
        for k in range(B):
            one = eng.icp_generalized_refine([srcs[k]], [dsts[k]], [inits[k]], constrained=constrained, **kw)
            for key in KEYS:
                assert np.array_equal(one[key][0], res[key][k]), (k, key)
        # other batch positions, and the rows form on the uploaded clouds out of order: bit-identical
        order = np.random.default_rng(5).permutation(B)
        moved = eng.icp_generalized_refine([srcs[k] for k in order], [dsts[k] for k in order], [inits[k] for k in order], constrained=constrained, **kw)
        rows = eng.icp_generalized_refine_rows(order, [inits[k] for k in order], constrained=constrained, **kw)
        for key in KEYS:
            assert np.array_equal(moved[key], res[key][order]), key
            assert np.array_equal(rows[key], res[key][order]), key
    assert skipped == 0          # (tests/test_icp_generalized_cpu.py::test_batch_inputs_are_decided_and_conditioned: the restatement leaves none undecided)
    eng.close()


def test_chunked_workspace_is_bit_identical(gpu_required):
    """The batch under a workspace budget of 1 MiB and of 64 KiB (option "icp_generalized_ws_budget"): many chunks, every chunk carved from offset 0 of
    the shared workspace -- the results of the one-chunk call, bit for bit, for both estimates.  The point-to-plane option is not read."""
    eng = _engine()
    srcs, dsts, inits = G.batch_pairs()
    kw = dict(radius=RADIUS, normal_radius=NORMAL_RADIUS, its=30)
    for constrained in (True, False):
        eng.set_option("icp_generalized_ws_budget", 0)
        one = eng.icp_generalized_refine(srcs, dsts, inits, constrained=constrained, **kw)
        assert eng.get_option("icp_generalized_chunks") == 1
        whole = eng.get_option("icp_grid_ws_bytes")
        chunks = []
        for budget in (1 << 20, 1 << 16):
            eng.set_option("icp_generalized_ws_budget", budget)
            eng.set_option("icp_plane_ws_budget", 1 << 12)
            cut = eng.icp_generalized_refine(srcs, dsts, inits, constrained=constrained, **kw)
            eng.set_option("icp_plane_ws_budget", 0)
            chunks.append(eng.get_option("icp_generalized_chunks"))
            assert eng.get_option("icp_grid_ws_bytes") < whole and eng.get_option("icp_generalized_ws_budget") == budget
            for key in KEYS:
                assert np.array_equal(cut[key], one[key]), (budget, key)
        print("constrained %d: one chunk of %d bytes; %s chunks under 1 MiB / 64 KiB" % (constrained, whole, chunks))
        assert 1 < chunks[0] < chunks[1] <= len(srcs)
    with pytest.raises(RuntimeError, match="icp_generalized_ws_budget"):
        eng.set_option("icp_generalized_ws_budget", -1)
    eng.close()


# ---- 3. the one-call registration -------------------------------------------------------------------------------------------------------------------
def test_register_generalized_equals_direct_call_from_own_network_transform(gpu_required):
    cfg = small_cfg(N=64, nb=12)
    spec, P32 = oracle_params(cfg)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    pairs = [P.corner_pair(n, 60 + i, constrained=i != 1) for i, n in enumerate((400, 900, 1500))]
    S, D = [p[0] for p in pairs], [p[1] for p in pairs]
    off = np.zeros((4, 2), np.int64)
    off[1:, 0] = np.cumsum([len(s) for s in S]); off[1:, 1] = np.cumsum([len(t) for t in D])
    eng.upload_dataset(np.concatenate(S), np.concatenate(D), off, np.zeros((3, 12), np.float32))
    rows = [2, 0, 1]
    hits = 0
    for constrained in (True, False):
        kw = dict(radius=1.0, normal_radius=NORMAL_RADIUS, its=12, constrained=constrained)      # (radius 1: an untrained network starts anywhere)
        host = eng.register(S, D, seed=11, refine="generalized", **kw)
        ref = eng.icp_generalized_refine(S, D, host["network_transforms"], **kw)
        dev = eng.register_rows(rows, 11, refine="generalized", **kw)
        ref_rows = eng.icp_generalized_refine_rows(rows, dev["network_transforms"], **kw)
        for key in KEYS:
            np.testing.assert_array_equal(host[key], ref[key], err_msg="host form, %s" % key)
            np.testing.assert_array_equal(dev[key], ref_rows[key], err_msg="rows form, %s" % key)
        np.testing.assert_array_equal(dev["transforms"], host["transforms"][rows])
        hits += int((host["fitness"] > 0.2).sum())
        assert not np.array_equal(host["transforms"], eng.register(S, D, seed=11, refine="plane", **kw)["transforms"])
    assert hits >= 2, "the refinement had nothing to refine: the comparison above would be vacuous"
    eng.close()


# ---- 4. errors, and the paths that do not change ------------------------------------------------------------------------------------------------------
def test_argument_errors_and_existing_paths_untouched(gpu_required):
    eng = _engine()
    src, dst, init, _ = P.corner_pair(700, 6)
    src2, dst2, init2 = _car()
    S, D, I = [src, src2], [dst, dst2], [init, init2]

    def existing():
        out = [eng.icp_refine(S, D, I, constrained=c) for c in (True, False)] + [eng.icp_plane_refine(S, D, I, constrained=c) for c in (True, False)]
        ev = eng.evaluate_registration(S, D, I, 0.1)
        return out, ev

    before, ev_before = existing()
    gen_before = [eng.icp_generalized_refine(S, D, I, constrained=c) for c in (True, False)]

    def check_unchanged():
        after, ev_after = existing()
        for b, a in zip(before + gen_before, after + [eng.icp_generalized_refine(S, D, I, constrained=c) for c in (True, False)]):
            for key in KEYS:
                assert np.array_equal(b[key], a[key]), key
        for key in ev_before:
            assert np.array_equal(np.asarray(ev_before[key]), np.asarray(ev_after[key])), key

    check_unchanged()
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(normal_radius=0.0), dict(normal_radius=float("nan")), dict(its=-1)):
        with pytest.raises(RuntimeError, match="radius|its"):
            eng.icp_generalized_refine(S, D, I, **bad)
    # flags: bit 0 only
    p1, p2 = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    off = np.array([[0, 0], [len(p1), len(p2)]], np.int64)
    T0, out = np.ascontiguousarray(init.reshape(16)), np.zeros(16)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for flags in (2, 3, 4, -1):
        rc = eng._lib.alignnet_icp_generalized_register(eng._h, fp(p1), fp(p2), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, dp(T0), 0.1, 0.3, 30, flags,
                                                        dp(out), None, None, None)
        assert rc != 0
        with pytest.raises(RuntimeError, match="unknown flags"):
            eng._check(rc)
    with pytest.raises(RuntimeError):
        eng.icp_generalized_refine_rows([0], [init])          # no dataset uploaded
    check_unchanged()
    eng.close()


# ---- 5. the drop-in -------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_icp_mode_with_generalized_estimate(gpu_required, tmp_path):
    """The ICP baseline mode (p2point from the centroid init): evaluation.icp_estimate = "generalized" registers by generalized ICP and writes the
    usual files; the environment wins."""
    sys.path.insert(0, PKG)
    import evaluation as EV
    from tests import icp_full_ref as F
    root = tmp_path / "SynthTiny"
    val = _make_dataset(str(root))
    ev = tmp_path / "logs" / "icp_SynthTiny" / "icp_SynthTiny_o3_p2p" / "val" / "eval000000"
    cfgp = tmp_path / "icp_SynthTiny_o3_p2p.json"
    got = {}
    for name, evaluation, extra in (("point", {"icp_estimate": "point"}, {}), ("generalized", {"icp_estimate": "generalized", "icp_normal_radius": 0.3}, {}),
                                    ("env", {"icp_estimate": "point"}, {"ALIGNNET_ICP_ESTIMATE": "generalized"})):
        json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
                   "evaluation": dict(evaluation, special={"mode": "icp", "icp": {"variant": "p2point", "with_constraint": True}})}, open(cfgp, "w"))
        out = _run(["train", "--config", str(cfgp)], str(tmp_path), **extra)
        assert ("ICP estimate: generalized" in out) == (name in ("generalized", "env")), out[-2000:]
        got[name] = {k: np.load(ev / ("%s.npy" % k)) for k in ("pred_translations", "pred_angles")}
    for k in ("pred_translations", "pred_angles"):
        assert np.array_equal(got["env"][k], got["generalized"][k])
        assert np.isfinite(got["generalized"][k]).all() and not np.array_equal(got["generalized"][k], got["point"][k])
    for k, (src, dst, _, truth) in enumerate(val):
        T = G.icp_generalized(src, dst, F.centroid_init(src, dst), 0.10, 0.3, 30, True)[0]
        np.testing.assert_allclose(got["generalized"]["pred_translations"][k], T[:3, 3], rtol=0, atol=1e-6)
        np.testing.assert_allclose(got["generalized"]["pred_angles"][k, 0], EV.rotvec_z(T[:3, :3]), rtol=0, atol=1e-6)


def test_train_py_refine_icp_with_generalized_estimate(gpu_required, tmp_path):
    """--refineICP from stored predictions near the truth (planted: two epochs of training predict nothing ICP could start from)."""
    root = tmp_path / "SynthTiny"
    val = _make_dataset(str(root))
    user = {"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
            "model": {"num_points": 64, "angles": {"num_bins": 12, "accept_inverted_angle": True},
                      "options": {"s1transformer": [[32, 64, 96], [[64, 32], 0.7]], "s2transformer": [[32, 64, 128], [[64, 32], 0.7]],
                                  "embedding": [32, 64, 160], "remaining_transform_prediction": [[64, 32], 0.7]}},
            "training": {"batch_size": 4, "num_epochs": 2, "learning_rate": 0.002}}
    cfgp = tmp_path / "GenRun.json"
    json.dump(user, open(cfgp, "w"))
    _run(["train", "--config", str(cfgp)], str(tmp_path))
    base = tmp_path / "logs" / "GenRun" / "val" / "eval000001"
    rng = np.random.default_rng(8)
    truth = np.stack([v[3] for v in val])
    np.save(base / "pred_translations.npy", (truth[:, :3, 3] + rng.normal(0, 0.02, (len(val), 3))).astype(np.float32))
    np.save(base / "pred_angles.npy", (np.arctan2(truth[:, 1, 0], truth[:, 0, 0]) + rng.normal(0, 0.01, len(val))).astype(np.float32).reshape(-1, 1))
    np.save(base / "pred_s2_pc1centers.npy", np.zeros((len(val), 3), np.float32))
    got = {}
    for estimate in ("point", "generalized"):
        json.dump(dict(user, evaluation={"icp_estimate": estimate, "icp_normal_radius": 0.3}), open(cfgp, "w"))
        out = _run(["eval_only", "--config", str(cfgp), "--eval_epoch", "1", "--refineICP", "--use_old_results"], str(tmp_path))
        assert ("ICP estimate: generalized" in out) == (estimate == "generalized")
        got[estimate] = {k: np.load(base / "refined_p2p" / ("%s.npy" % k)) for k in ("pred_translations", "pred_angles")}
    for k in ("pred_translations", "pred_angles"):
        assert np.isfinite(got["generalized"][k]).all() and not np.array_equal(got["generalized"][k], got["point"][k])
    err = lambda g: np.abs(g["pred_translations"] - truth[:, :3, 3]).max()
    print("--refineICP: largest translation error, point %.2f mm, generalized %.2f mm" % (1e3 * err(got["point"]), 1e3 * err(got["generalized"])))
    assert err(got["generalized"]) < 0.02 and err(got["point"]) < 0.05       # both land near the truth they started 2 cm from
