"""GPU: point-to-plane ICP (Engine.icp_plane_refine*, csrc/alignnet_icp.hip: icp_plane_sort_kernel, icp_plane_normals_kernel, icp_surface_kernel<false, .>)
against the fp64 restatement tests/icp_plane_ref.py.  Stage by stage through Engine.debug_icp_plane (the shipped source compiled with a record behind
it), every stage fed the DEVICE's own upstream outputs: neighbour counts equal, normals to 1e-8, index / inlier / fitness equal, squared distances and
residuals to 1e-12 relative, every sum within 4 n u sum |term| (the rounding bound of an n-term fp64 sum, u = 2^-53), the update within 1e-9 of the
restatement's solve of the device's sums.  Whole runs to the bars of tests/test_icp_gpu.py / test_icp_scan_gpu.py: transforms within
1e-9 max(1, |offset|), rmse within 1e-9, fitness and iteration counts equal.  An entry within the margins of a decision (P.UNDECIDED, P.UNDECIDED_GAP)
is left out of its stage's comparison; at most P.SKIP_CAP of a stage's entries may be."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alignnet3d
from oracle import alignnet_ref as R
from tests import icp_plane_ref as P
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
RADIUS, NORMAL_RADIUS = 0.1, 0.3


def _engine():
    return alignnet3d.Engine(small_cfg(N=64, nb=12))


def _stages(eng, name, src, dst, T, tally, radius=RADIUS, normal_radius=NORMAL_RADIUS):
    """One pair through the read-back, both estimates.  tally: [normals skipped, normals, points skipped, points]."""
    dst64 = np.asarray(dst, np.float64).reshape(-1, 3)
    nr = P.normals(dst, normal_radius)
    und_n = P.normals_undecided(nr)
    e = P.evaluate(src, dst, T, radius) if len(dst) and len(src) else None
    tally[0] += int(und_n.sum()); tally[1] += len(dst)
    out = {}
    for constrained in (True, False):
        full = not constrained
        d = eng.debug_icp_plane(src, dst, T, radius=radius, normal_radius=normal_radius, constrained=constrained)
        out[constrained] = d
        # 1. normals
        sure = nr["nbr_margin"] >= P.UNDECIDED
        assert np.array_equal(d["neighbours"][sure], nr["count"][sure]), (name, "neighbour counts")
        nerr = np.abs(d["normals"] - nr["normals"]).max(1) if len(dst) else np.zeros(0)
        print("%s constrained %d: n1 %d n2 %d, neighbours mean %.1f max %d, normals undecided %d, worst normal error %.3g"
              % (name, constrained, len(src), len(dst), d["neighbours"].mean() if len(dst) else 0, d["neighbours"].max() if len(dst) else 0, und_n.sum(),
                 nerr[~und_n].max() if (~und_n).any() else 0.0))
        assert np.all(nerr[~und_n] <= 1e-8), (name, "normals")
        assert np.all(d["normals"][:, 2] >= 0) and np.array_equal(d["normals"][d["neighbours"] < 3], np.tile([0.0, 0.0, 1.0], (int((d["neighbours"] < 3).sum()), 1)))
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
        # 3. residuals of the device's inliers from the device's index and normals
        di = d["inlier"]
        j = d["index"][di]
        r = P.residuals(e["p"][di], dst64[j], d["normals"][j])
        rerr = np.abs(d["residual"][di] - r)
        print("   fitness %.4f, %d undecided points, worst relative dist2 error %.3g, worst residual error %.3g (smallest |residual| %.3g)"
              % (d["fitness"], (~ok).sum(), rel.max() if rel.size else 0, rerr.max() if rerr.size else 0, np.abs(r).min() if r.size else 0))
        assert np.all(rerr <= 1e-12 * np.abs(r)), (name, "residuals")
        assert not d["residual"][~di].any()
        # 4. the sums, of the device's correspondences, normals and distances
        c = dst64[0]
        s, mag, n = P.sums(e["p"][di], dst64[j], d["normals"][j], d["dist2"][di], c, full)
        bound = 4.0 * n * P.U64 * mag
        assert d["sums"][0] == n and np.all(np.abs(d["sums"] - s) <= bound), (name, "sums", np.abs(d["sums"] - s), bound)
        assert not d["sums"][P.nsums(full):].any()
        assert abs(d["rmse"] - (np.sqrt(d["sums"][1] / n) if n else 0.0)) <= 1e-15
        # 5. the update, from the device's sums
        info = {}
        U, det = P.solve(d["sums"], c, full, info)
        print("   update: determined %d, scaled condition number %.3g, error %.3g" % (det, info["cond"], np.abs(d["update"] - U).max()))
        assert det or np.array_equal(d["update"], np.eye(4)), (name, "an undetermined update is the identity")
        assert not det or info["cond"] <= 1e4, (name, "the inputs are to be well conditioned or exactly singular", info["cond"])
        np.testing.assert_allclose(d["update"], U, rtol=0, atol=1e-9, err_msg=name)
    return out


@functools.lru_cache(maxsize=None)
def _car():
    src, dst, truth = P.car_pair(10.0, 1, scale=4.4)
    return src, dst, P.disturbed(truth, src.astype(np.float64).mean(0), seed=1)


# ---- 1. stage parity ------------------------------------------------------------------------------------------------------------------------------
def test_stages_corner_car_and_far_frame(gpu_required):
    eng = _engine()
    tally = [0, 0, 0, 0]
    src, dst, init, _ = P.corner_pair(300, 1, constrained=False)
    _stages(eng, "corner 300", src, dst, init, tally)
    src, dst, init = _car()                                                   # about 4,700 targets in a few dozen cells: many records per cell
    _stages(eng, "car scan", src, dst, init, tally)
    src, dst, init, _ = P.corner_pair(2000, 2, offset=5000.0, constrained=False, side=2.5)   # 5 km out: float32 coordinates on a 0.5 mm lattice
    _stages(eng, "corner 5 km", src, dst, init, tally)
    assert tally[0] <= P.SKIP_CAP * tally[1] and tally[2] <= P.SKIP_CAP * tally[3], tally
    eng.close()


def test_stages_large_target(gpu_required):
    """40,001 targets: beyond the 32,768-bucket cap of the hashed grid, several workgroups of the normals kernel, n2 no multiple of its block."""
    eng = _engine()
    tally = [0, 0, 0, 0]
    src, dst, init, _ = P.corner_pair(40001, 3, constrained=False, side=6.0)
    d = _stages(eng, "corner 40001", src[:1500], dst, init, tally)
    assert d[True]["fitness"] > 0.5
    assert tally[0] <= P.SKIP_CAP * tally[1] and tally[2] <= P.SKIP_CAP * tally[3], tally
    eng.close()


def test_stages_strays_and_size_edges(gpu_required):
    eng = _engine()
    tally = [0, 0, 0, 0]
    src, dst, init, _ = P.corner_pair(300, 4)
    base = dst.astype(np.float64).mean(0)
    strays = np.array([[4.0, 0, 0], [0, 5.0, 0], [0, 5.12, 0.01], [0, 0, 6.0], [0.11, 0, 6.0], [-4.0, 0.2, 0]]) + base     # K = 1, 2, 2, 2, 2, 1
    dst2 = np.concatenate([dst, strays.astype(np.float32)])
    inv = np.linalg.inv(init)
    near = ((strays + [0.01, -0.02, 0.015]) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)                               # sources that land on the strays
    d = _stages(eng, "strays", np.concatenate([src, near]), dst2, init, tally)[True]
    assert d["neighbours"][300:].tolist() == [1, 2, 2, 2, 2, 1] and d["inlier"][-6:].all() and np.array_equal(d["index"][-6:], 300 + np.arange(6))
    for n2 in (0, 1, 2, 3):
        _stages(eng, "n2 %d" % n2, src[:40], dst[:n2], init, tally)
    _stages(eng, "empty source", src[:0], dst, init, tally)
    assert tally[0] <= P.SKIP_CAP * tally[1] and tally[2] <= P.SKIP_CAP * tally[3], tally
    eng.close()


@pytest.mark.parametrize("tilt", [(0.0, 0.0), (0.25, -0.125)])
def test_single_plane_determines_no_update(gpu_required, tilt):
    eng = _engine()
    src, dst = P.plane_pair(600, 4, tilt)
    tally = [0, 0, 0, 0]
    d = _stages(eng, "plane %s" % (tilt,), src, dst, np.eye(4), tally)
    for constrained in (True, False):
        assert np.array_equal(d[constrained]["update"], np.eye(4)) and d[constrained]["fitness"] > 0.9
        ref = P.icp_plane(src, dst, np.eye(4), RADIUS, NORMAL_RADIUS, 30, constrained)
        res = eng.icp_plane_refine([src], [dst], [np.eye(4)], constrained=constrained)
        assert np.array_equal(res["transforms"][0], np.eye(4)) and res["iterations"][0] == 1 == ref[3] and res["fitness"][0] == ref[1]
    eng.close()


# ---- 2. whole runs ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_reference(constrained):
    srcs, dsts, inits = P.batch_pairs()
    out = []
    for s, d, i in zip(srcs, dsts, inits):
        info = {}
        out.append(P.icp_plane(s, d, i, RADIUS, NORMAL_RADIUS, 30, constrained, info=info) + (info,))
    return out


def test_whole_runs_batch_alone_and_dataset(gpu_required):
    eng = _engine()
    srcs, dsts, inits = P.batch_pairs()
    B = len(srcs)
    off = np.zeros((B + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(s) for s in srcs]); off[1:, 1] = np.cumsum([len(t) for t in dsts])
    eng.upload_dataset(np.concatenate(srcs), np.concatenate(dsts), off, np.zeros((B, 12), np.float32))
    skipped = 0
    for constrained in (True, False):
        res = eng.icp_plane_refine(srcs, dsts, inits, radius=RADIUS, normal_radius=NORMAL_RADIUS, its=30, constrained=constrained)
        refs = _batch_reference(constrained)
        for k in range(B):
            T, fit, rmse, it, und, info = refs[k]
            conds = [c for c, ok in zip(info.get("conds", []), info.get("determined", [])) if ok]
            assert not conds or max(conds) <= 1e4, (k, "the inputs are to be well conditioned or exactly singular")
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
            one = eng.icp_plane_refine([srcs[k]], [dsts[k]], [inits[k]], radius=RADIUS, normal_radius=NORMAL_RADIUS, its=30, constrained=constrained)
            for key in ("transforms", "fitness", "rmse", "iterations"):
                assert np.array_equal(one[key][0], res[key][k]), (k, key)
        # the rows form on the uploaded clouds, out of order: bit-identical to the host form
        order = np.random.default_rng(5).permutation(B)
        rows = eng.icp_plane_refine_rows(order, [inits[k] for k in order], radius=RADIUS, normal_radius=NORMAL_RADIUS, its=30, constrained=constrained)
        for key in ("transforms", "fitness", "rmse", "iterations"):
            assert np.array_equal(rows[key], res[key][order]), key
    assert skipped == 0          # (tests/test_icp_plane_cpu.py::test_batch_inputs_are_decided_and_conditioned: the restatement leaves none undecided)
    eng.close()


def test_chunked_workspace_is_bit_identical(gpu_required):
    """The batch under a workspace budget of 1 MiB and of 64 KiB (option "icp_plane_ws_budget"): many chunks, the pairs above the budget alone in
    theirs, every chunk carved from offset 0 of the shared workspace -- the results of the one-chunk call, bit for bit, for both estimates."""
    eng = _engine()
    srcs, dsts, inits = P.batch_pairs()
    for constrained in (True, False):
        eng.set_option("icp_plane_ws_budget", 0)
        one = eng.icp_plane_refine(srcs, dsts, inits, radius=RADIUS, normal_radius=NORMAL_RADIUS, its=30, constrained=constrained)
        assert eng.get_option("icp_plane_chunks") == 1
        whole = eng.get_option("icp_grid_ws_bytes")
        chunks = []
        for budget in (1 << 20, 1 << 16):
            eng.set_option("icp_plane_ws_budget", budget)
            cut = eng.icp_plane_refine(srcs, dsts, inits, radius=RADIUS, normal_radius=NORMAL_RADIUS, its=30, constrained=constrained)
            chunks.append(eng.get_option("icp_plane_chunks"))
            assert eng.get_option("icp_grid_ws_bytes") < whole
            for key in ("transforms", "fitness", "rmse", "iterations"):
                assert np.array_equal(cut[key], one[key]), (budget, key)
        print("constrained %d: one chunk of %d bytes; %s chunks under 1 MiB / 64 KiB" % (constrained, whole, chunks))
        assert 1 < chunks[0] < chunks[1] <= len(srcs)
    with pytest.raises(RuntimeError, match="icp_plane_ws_budget"):
        eng.set_option("icp_plane_ws_budget", -1)
    eng.close()


# ---- 3. flags, and the paths that do not change -------------------------------------------------------------------------------------------------------
def test_unknown_flags_and_point_path_untouched(gpu_required):
    import ctypes as C
    eng = _engine()
    src, dst, init, _ = P.corner_pair(700, 6)
    src2, dst2, init2 = _car()
    before = [eng.icp_refine([src, src2], [dst, dst2], [init, init2], constrained=c) for c in (True, False)]
    eng.set_option("icp_search", 1)
    before += [eng.icp_refine([src, src2], [dst, dst2], [init, init2], constrained=c) for c in (True, False)]
    for c in (True, False):
        eng.icp_plane_refine([src2, src], [dst2, dst], [init2, init], constrained=c)
    after = [eng.icp_refine([src, src2], [dst, dst2], [init, init2], constrained=c) for c in (True, False)]
    eng.set_option("icp_search", 0)
    after = [eng.icp_refine([src, src2], [dst, dst2], [init, init2], constrained=c) for c in (True, False)] + after
    for b, a in zip(before, after):
        for key in ("transforms", "fitness", "rmse", "iterations"):
            assert np.array_equal(b[key], a[key]), key
    # flags: bit 0 only
    p1, p2 = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    off = np.array([[0, 0], [len(p1), len(p2)]], np.int64)
    T0, out = np.ascontiguousarray(init.reshape(16)), np.zeros(16)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for flags in (2, 3, 4, -1):
        rc = eng._lib.alignnet_icp_plane_register(eng._h, fp(p1), fp(p2), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, dp(T0), 0.1, 0.3, 30, flags, dp(out),
                                                  None, None, None)
        assert rc != 0
        with pytest.raises(RuntimeError, match="unknown flags"):
            eng._check(rc)
    with pytest.raises(RuntimeError, match="normal_radius"):
        eng.icp_plane_refine([src], [dst], [init], normal_radius=0.0)
    eng.close()


# ---- 4. the drop-in -------------------------------------------------------------------------------------------------------------------------------------
def _make_dataset(root, n=20, seed=40):
    """On-disk layout of tests/test_dropin_gpu.py::_make_dataset with noisy box corners of 300 to 600 points (surfaces: the normals mean something),
    sources a 70 % subset moved about z; val = the last 8.  Returns the val pairs and their true transforms."""
    rng = np.random.default_rng(seed)
    pairs = [P.corner_pair(int(rng.integers(300, 600)), seed + i, constrained=True) for i in range(n)]
    for sub in ("meta", "pointcloud1", "pointcloud2", "split"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    txt = lambda v: "\n".join("%.18e" % x for x in np.ravel(v)) + "\n"
    for i, (src, dst, _, truth) in enumerate(pairs):
        c1 = src.astype(np.float64).mean(0)
        meta = {"translation": txt(truth[:3, 3]), "rel_angle": float(np.arctan2(truth[1, 0], truth[0, 0])),
                "start_position": txt(c1), "end_position": txt(truth[:3, :3] @ c1 + truth[:3, 3]), "start_angle": 0.0, "end_angle": 0.0}
        json.dump(meta, open(os.path.join(root, "meta", "%08d.json" % i), "w"))
        np.save(os.path.join(root, "pointcloud1", "%08d.npy" % i), src)
        np.save(os.path.join(root, "pointcloud2", "%08d.npy" % i), dst)
    open(os.path.join(root, "split", "train.txt"), "w").write("\n".join(map(str, range(12))) + "\n")
    open(os.path.join(root, "split", "val.txt"), "w").write("\n".join(map(str, range(12, n))) + "\n")
    return pairs[12:]


def _run(args, cwd, **extra):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    env.pop("ALIGNNET_ICP_ESTIMATE", None)
    env.pop("ALIGNNET_ICP_SEARCH", None)
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py")] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def test_train_py_icp_mode_with_plane_estimate(gpu_required, tmp_path):
    """The ICP baseline mode (p2point from the centroid init): evaluation.icp_estimate = "plane" registers by point-to-plane, an absent key or "point"
    writes today's files bit for bit, the environment wins."""
    sys.path.insert(0, PKG)
    import evaluation as EV
    from tests import icp_full_ref as F
    root = tmp_path / "SynthTiny"
    val = _make_dataset(str(root))
    ev = tmp_path / "logs" / "icp_SynthTiny" / "icp_SynthTiny_o3_p2p" / "val" / "eval000000"
    cfgp = tmp_path / "icp_SynthTiny_o3_p2p.json"
    got = {}
    for name, evaluation, extra in ((None, {}, {}), ("point", {"icp_estimate": "point"}, {}), ("plane", {"icp_estimate": "plane", "icp_normal_radius": 0.3}, {}),
                                    ("env", {"icp_estimate": "point"}, {"ALIGNNET_ICP_ESTIMATE": "plane"})):
        json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
                   "evaluation": dict(evaluation, special={"mode": "icp", "icp": {"variant": "p2point", "with_constraint": True}})}, open(cfgp, "w"))
        out = _run(["train", "--config", str(cfgp)], str(tmp_path), **extra)
        assert ("ICP estimate: point-to-plane" in out) == (name in ("plane", "env")), out[-2000:]
        got[name] = {k: np.load(ev / ("%s.npy" % k)) for k in ("pred_translations", "pred_angles")}
    for k in ("pred_translations", "pred_angles"):
        assert np.array_equal(got[None][k], got["point"][k]) and np.array_equal(got["env"][k], got["plane"][k])
        assert np.isfinite(got["plane"][k]).all() and not np.array_equal(got["plane"][k], got["point"][k])
    for k, (src, dst, _, truth) in enumerate(val):
        init = F.centroid_init(src, dst)
        T = P.icp_plane(src, dst, init, 0.10, 0.3, 30, True)[0]
        np.testing.assert_allclose(got["plane"]["pred_translations"][k], T[:3, 3], rtol=0, atol=1e-6)
        np.testing.assert_allclose(got["plane"]["pred_angles"][k, 0], EV.rotvec_z(T[:3, :3]), rtol=0, atol=1e-6)
        Tz = F.icp_p2point(src, dst, init, 0.10, 30, with_constraint=True)[0]
        np.testing.assert_allclose(got[None]["pred_translations"][k], Tz[:3, 3], rtol=0, atol=1e-6)


def test_train_py_refine_icp_with_plane_estimate(gpu_required, tmp_path):
    """--refineICP from stored predictions near the truth (planted: two epochs of training predict nothing ICP could start from)."""
    root = tmp_path / "SynthTiny"
    val = _make_dataset(str(root))
    user = {"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
            "model": {"num_points": 64, "angles": {"num_bins": 12, "accept_inverted_angle": True},
                      "options": {"s1transformer": [[32, 64, 96], [[64, 32], 0.7]], "s2transformer": [[32, 64, 128], [[64, 32], 0.7]],
                                  "embedding": [32, 64, 160], "remaining_transform_prediction": [[64, 32], 0.7]}},
            "training": {"batch_size": 4, "num_epochs": 2, "learning_rate": 0.002}}
    cfgp = tmp_path / "PlaneRun.json"
    json.dump(user, open(cfgp, "w"))
    _run(["train", "--config", str(cfgp)], str(tmp_path))
    base = tmp_path / "logs" / "PlaneRun" / "val" / "eval000001"
    rng = np.random.default_rng(8)
    truth = np.stack([v[3] for v in val])
    np.save(base / "pred_translations.npy", (truth[:, :3, 3] + rng.normal(0, 0.02, (len(val), 3))).astype(np.float32))
    np.save(base / "pred_angles.npy", (np.arctan2(truth[:, 1, 0], truth[:, 0, 0]) + rng.normal(0, 0.01, len(val))).astype(np.float32).reshape(-1, 1))
    np.save(base / "pred_s2_pc1centers.npy", np.zeros((len(val), 3), np.float32))
    got = {}
    for estimate in (None, "point", "plane"):
        if estimate:
            json.dump(dict(user, evaluation={"icp_estimate": estimate, "icp_normal_radius": 0.3}), open(cfgp, "w"))
        out = _run(["eval_only", "--config", str(cfgp), "--eval_epoch", "1", "--refineICP", "--use_old_results"], str(tmp_path))
        assert ("ICP estimate: point-to-plane" in out) == (estimate == "plane")
        got[estimate] = {k: np.load(base / "refined_p2p" / ("%s.npy" % k)) for k in ("pred_translations", "pred_angles")}
    for k in ("pred_translations", "pred_angles"):
        assert np.isfinite(got["plane"][k]).all()
        assert np.array_equal(got[None][k], got["point"][k])          # an absent key: the files of the point-to-point refinement, bit for bit
        assert not np.array_equal(got["plane"][k], got["point"][k])
    err = lambda g: np.abs(g["pred_translations"] - truth[:, :3, 3]).max()
    print("--refineICP: largest translation error, point %.2f mm, plane %.2f mm" % (1e3 * err(got["point"]), 1e3 * err(got["plane"])))
    assert err(got["plane"]) < 0.02 and err(got["point"]) < 0.05       # both land near the truth they started 2 cm from
