"""CPU: generalized (plane-to-plane) ICP as restated in tests/icp_generalized_ref.py (the definition of alignnet_icp_generalized_register*), the
declaration and binding of the new C entry points, and the drop-in's option.  No compute calls (there is no GPU and no CPU fallback)."""
import functools
import os
import re
import sys
import types

import numpy as np
import pytest

from oracle import icp_ref
from tests import icp_generalized_ref as G
from tests import icp_plane_ref as P
from tests.test_icp_plane_cpu import SCENE_SCALE, SCENE_SEEDS, SCENE_STRIDE, _corner_correspondences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_and_bound():
    from alignnet3d import _capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alignnet_hip.h")).read(), flags=re.S)
    names = (("alignnet_icp_generalized_register", 14), ("alignnet_icp_generalized_register_dataset", 12), ("alignnet_debug_icp_generalized", 20))
    for name, nargs in names:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, name + " not declared in include/alignnet_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_capi.SYMBOLS[name][1]), name
    # the generalized entry points take what the point-to-plane ones take
    for a, b in (("alignnet_icp_generalized_register", "alignnet_icp_plane_register"),
                 ("alignnet_icp_generalized_register_dataset", "alignnet_icp_plane_register_dataset")):
        assert _capi.SYMBOLS[a] == _capi.SYMBOLS[b]
    import alignnet3d
    lib = alignnet3d.load_library()
    for name, _ in names:
        assert hasattr(lib, name)
    for method in ("icp_generalized_refine", "icp_generalized_refine_rows", "debug_icp_generalized"):
        assert callable(getattr(alignnet3d.Engine, method))
    assert alignnet3d.Engine.REFINE["generalized"] not in (0, 1, 2) and "generalized" in alignnet3d.Engine.REFINE
    assert {"icp_generalized_normals", "icp_generalized"} <= set(alignnet3d.Engine.PROFILED_KERNELS)


def test_icp_estimate_option():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import train

    def conf(**ev):
        return types.SimpleNamespace(evaluation=types.SimpleNamespace(**ev))

    assert train.icp_estimate_option(conf(icp_estimate="generalized"), {}) == ("generalized", 0.3)
    assert train.icp_estimate_option(conf(icp_estimate="generalized", icp_normal_radius=0.25), {}) == ("generalized", 0.25)
    assert train.icp_estimate_option(conf(), {"ALIGNNET_ICP_ESTIMATE": "generalized"}) == ("generalized", 0.3)
    assert train.icp_estimate_option(conf(icp_estimate="generalized"), {"ALIGNNET_ICP_ESTIMATE": "point"}) == ("point", 0.3)
    assert train.icp_estimate_option(conf(), {}) == ("point", 0.3)                 # the default stays
    for bad in ("p2plane", "Plane ", "1", "gicp"):
        with pytest.raises(ValueError, match="point, plane, generalized"):
            train.icp_estimate_option(conf(icp_estimate=bad), {})
    with pytest.raises(ValueError, match="icp_normal_radius"):
        train.icp_estimate_option(conf(icp_estimate="generalized", icp_normal_radius=0.0), {})
    import register_pair
    assert register_pair.parse_args(["--config", "c", "--model", "m", "--source", "a", "--target", "b", "--refine", "generalized"]).refine == "generalized"
    assert register_pair.REFINE["generalized"] == "generalized"


# ---- the weight matrix -------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _normal_pairs():
    rng = np.random.default_rng(11)
    nq = _unit(rng.normal(size=(400, 3)))
    m = _unit(rng.normal(size=(400, 3)))
    m[:50] = nq[:50]                                              # n_q = m
    m[50:100] = _unit(np.cross(nq[50:100], rng.normal(size=(50, 3))))   # n_q perpendicular to m
    m[100:120] = -nq[100:120]
    nq[120] = m[120] = [0.0, 0.0, 1.0]                           # the default normal of both
    return nq, m


def test_covariance_sum_spectrum_and_closed_form_inverse():
    nq, m = _normal_pairs()
    A = G.cov_sum(nq, m)
    w = np.linalg.eigvalsh(A)
    slack = 8 * G.U64 * 2.0
    assert w.min() >= 2 * G.EPS - slack and w.max() <= 2.0 + slack, (w.min(), w.max())
    assert np.allclose(w[:50, 0], 2 * G.EPS, rtol=0, atol=1e-14) and np.allclose(w[:50, 1:], 2.0, rtol=0, atol=1e-14)              # n_q = m
    assert np.allclose(w[50:100], [1 + G.EPS, 1 + G.EPS, 2.0], rtol=0, atol=1e-13)                                                  # n_q perp m
    assert np.allclose(A, np.swapaxes(A, 1, 2))
    M = G.inverse3(A)
    ref = np.linalg.inv(A)
    rel = np.abs(M - ref).max((1, 2)) / np.abs(ref).max((1, 2))
    print("closed-form inverse against numpy.linalg.inv: worst relative error %.3g, largest |M| %.4g" % (rel.max(), np.abs(M).max()))
    assert rel.max() <= 1e-12
    along = np.einsum("ni,nij,nj->n", nq[:50], M[:50], nq[:50])
    assert np.abs(along - 0.5 / G.EPS).max() < 1e-9                           # 1 / (2 eps) along the shared normal


# ---- the estimate ------------------------------------------------------------------------------------------------------------------------------
def _delta(x, c, full):
    """Delta(x) = Tr(c) [Rz Ry Rx | t] Tr(-c): the update as the solve composes it."""
    return P.rigid_about(c, (x[0], x[1], x[2]) if full else (0.0, 0.0, x[0]), np.asarray(x[3:] if full else x[1:]))


@pytest.mark.parametrize("full", [False, True])
def test_gauss_newton_step_against_central_differences(full):
    """One step of the estimate equals the least-squares step of a numerically differentiated residual L^T (Delta(x) p - q), M = L L^T held fixed:
    the signs of J, the order of its columns and the composition of the update, from something that shares no formula with them."""
    rng = np.random.default_rng(21)
    n = 300
    c = np.array([3.2, -1.7, 0.9])
    q = c + rng.uniform(-1.5, 1.5, (n, 3))
    T = P.rigid_about(c, (0.02, -0.03, 0.05), np.array([0.01, 0.02, -0.015]))
    src = (q + rng.normal(0, 0.01, (n, 3)) - T[:3, 3]) @ T[:3, :3]          # T src = q + noise
    p = P.transform(src, T)
    nq, n_p = _unit(rng.normal(size=(n, 3))), _unit(rng.normal(size=(n, 3)))
    M = G.weights(nq, n_p, T)
    L = np.linalg.cholesky(M)
    best = ((p - q) ** 2).sum(1)
    s = G.sums(p, q, nq, n_p, T, best, c, full)[0]
    info = {}
    U, ok = P.solve(s, c, full, info)
    assert ok
    N = 6 if full else 4

    def resid(x):
        D = _delta(x, c, full)
        d = p @ D[:3, :3].T + D[:3, 3] - q
        return np.einsum("nji,nj->ni", L, d).ravel()

    def cost(x):
        D = _delta(x, c, full)
        return G.objective(p @ D[:3, :3].T + D[:3, 3], q, M)

    h = 1e-6
    Jr = np.stack([(resid(h * np.eye(N)[k]) - resid(-h * np.eye(N)[k])) / (2 * h) for k in range(N)], 1)
    grad = np.array([(cost(h * np.eye(N)[k]) - cost(-h * np.eye(N)[k])) / (2 * h) for k in range(N)])
    g = s[2 + len(G.TRI[full]): 2 + len(G.TRI[full]) + N]
    assert np.abs(grad - 2 * g).max() <= 1e-6 * np.abs(g).max(), (grad, 2 * g)                # the gradient of sum d^T M d is 2 J^T M d
    A = np.zeros((N, N))
    for k, (i, j) in enumerate(G.TRI[full]):
        A[i, j] = A[j, i] = s[2 + k]
    assert np.abs(Jr.T @ Jr - A).max() <= 1e-6 * np.abs(A).max()
    x_fd = -np.linalg.lstsq(Jr, resid(np.zeros(N)), rcond=None)[0]
    print("full %d: step %s, against finite differences %.3g" % (full, info["x"], np.abs(info["x"] - x_fd).max()))
    assert np.abs(info["x"] - x_fd).max() <= 1e-6 * np.abs(x_fd).max()
    assert np.abs(U - _delta(info["x"], c, full)).max() <= 1e-14
    assert cost(info["x"]) < cost(np.zeros(N))                                                # and the step goes downhill


@pytest.mark.parametrize("full", [False, True])
def test_estimate_recovers_a_small_motion_to_second_order(full):
    c = np.array([3.2, -1.7, 0.9])
    for angle in (1e-2, 1e-3):
        ang = np.array([0.6, -0.8, 1.0]) * angle * ([1, 1, 1] if full else [0, 0, 1])
        motion = P.rigid_about(c, ang, np.array([0.004, -0.003, 0.002]))
        p, q, nrm = _corner_correspondences(600, 5, motion)
        n_p = nrm @ motion[:3, :3]                                   # the faces' normals in the source's frame: R^T n
        best = ((p - q) ** 2).sum(1)
        s, mag, n = G.sums(p, q, nrm, n_p, np.eye(4), best, c, full)
        info = {}
        U, ok = P.solve(s, c, full, info)
        assert ok and info["cond"] < 1e3
        err = np.abs(U - motion).max()
        print("full %d angle %g: update error %.3g (angle^2 = %.3g), cond %.3g" % (full, angle, err, angle ** 2, info["cond"]))
        assert err < 6.0 * angle ** 2, (angle, err)


@pytest.mark.parametrize("tilt", [(0.0, 0.0), (0.25, -0.125)])
@pytest.mark.parametrize("constrained", [True, False])
def test_single_plane_is_regular(constrained, tilt):
    """Where point-to-plane determines nothing, every generalized estimate is determined and the run ends at the planted shift."""
    src, dst = P.plane_pair(600, 4, tilt)
    init = np.eye(4)
    info = {}
    T, fit, rmse, k, und = G.icp_generalized(src, dst, init, 0.1, 0.3, 30, constrained, info=info)
    print("tilt %s constrained %d: %d iterations, conds %s, T - planted %.3g" % (tilt, constrained, k, ["%.3g" % c for c in info["conds"]],
                                                                               np.abs(T - P.rigid_about(np.zeros(3), (0, 0, 0), np.array([0, 0, -0.03]))).max()))
    assert all(info["determined"]) and max(info["conds"]) <= 1e4
    assert k <= 5 and fit > 0.9
    assert np.abs(T - P.rigid_about(np.zeros(3), (0.0, 0.0, 0.0), np.array([0.0, 0.0, -0.03]))).max() <= 1e-6
    pinfo = {}
    Tp = P.icp_plane(src, dst, init, 0.1, 0.3, 30, constrained, info=pinfo)[0]
    assert pinfo["determined"] == [False] and np.array_equal(Tp, init)


# ---- scene pairs -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene_run(seed):
    src, dst, truth = P.car_pair(10.0, seed, scale=SCENE_SCALE)
    src = src[::SCENE_STRIDE]
    centre = src.astype(np.float64).mean(0)
    init = P.disturbed(truth, centre, seed=seed)
    nq, n_p = P.normals(dst, 0.3), P.normals(src, 0.3)
    info = {}
    res = G.icp_generalized(src, dst, init, 0.1, 0.3, 30, True, nrm_dst=nq, nrm_src=n_p, info=info)
    return src, dst, truth, init, centre, nq, n_p, info, res


@pytest.mark.parametrize("seed", SCENE_SEEDS)
def test_scene_pairs_generalized_beats_point(seed):
    """The car pairs of tests/test_icp_plane_cpu.py: noisy scans at scale 4.4, 10 m out, from the truth turned by 4 degrees and shifted 0.12 m."""
    src, dst, truth, init, centre, nq, n_p, info, (T, fit, rmse, k, und) = _scene_run(seed)
    Tz, fz, rz, kz = icp_ref.icp_p2point_z(src, dst, init, 0.1, 30)
    (yaw, tr), (yawz, trz), (yaw0, tr0) = P.pose_error(T, truth, centre), P.pose_error(Tz, truth, centre), P.pose_error(init, truth, centre)
    print("seed %d: n1 %d n2 %d; init %.2f deg %.1f mm; generalized %d its %.3f deg %.2f mm fitness %.4f; point %d its %.3f deg %.2f mm fitness %.4f; "
          "cond max %.3g" % (seed, len(src), len(dst), yaw0, tr0 * 1e3, k, yaw, tr * 1e3, fit, kz, yawz, trz * 1e3, fz, max(info["conds"])))
    assert k < 30                                         # ends within the iteration limit
    assert tr < trz                                       # nearer the truth than point-to-point from the same start
    assert all(info["determined"]) and max(info["conds"]) <= 1e4


def test_undecided_share_of_the_restatement():
    """Both clouds' normals and the correspondences: the restatement alone stays at or below REF_CAP undecided entries per stage."""
    for seed in SCENE_SEEDS:
        src, dst, truth, init, centre, nq, n_p, info, (T, fit, rmse, k, und) = _scene_run(seed)
        share_q, share_p = float(P.normals_undecided(nq).mean()), float(P.normals_undecided(n_p).mean())
        share_e = float(P.evaluate(src, dst, init, 0.1)["undecided"].mean())
        print("seed %d: undecided target normals %.2e, source normals %.2e, correspondences %.2e, over the run %d entries"
              % (seed, share_q, share_p, share_e, und))
        assert share_q <= P.REF_CAP and share_p <= P.REF_CAP and share_e <= P.REF_CAP
        assert und <= P.REF_CAP * (info["evaluations"] * len(src))


def test_batch_inputs_are_decided_and_conditioned():
    """The pairs of the GPU whole-run test: the restatement leaves at most REF_CAP of its entries undecided, and every estimate is either without
    correspondences or has a scaled condition number <= 1e4 -- the single planes included.  P.batch_pairs() does not meet this: its planes of 1, 2
    and 3 targets give one or two correspondences, which leave a rotation exactly undetermined (shown first); G.batch_pairs() replaces them by
    planes of 8, 12 and 20 targets and keeps everything else."""
    srcs, dsts, inits = P.batch_pairs()
    for k in (3, 5, 7):
        info = {}
        fit = G.icp_generalized(srcs[k], dsts[k], inits[k], 0.1, 0.3, 30, False, info=info)[1]
        assert fit == 1.0 and info["determined"] == [False], (k, info)
    srcs, dsts, inits = G.batch_pairs()
    assert len(srcs) == 70 and min(map(len, dsts)) == 0 and max(map(len, dsts)) >= 6000 and any(len(s) == 0 and len(d) for s, d in zip(srcs, dsts))
    assert sum(0 < len(d) < 63 for d in dsts) == 15
    worst, und_all, entries = 0.0, 0, 0
    for constrained in (True, False):
        for k, (s, d, i) in enumerate(zip(srcs, dsts, inits)):
            info = {}
            T, fit, rmse, it, und = G.icp_generalized(s, d, i, 0.1, 0.3, 30, constrained, info=info)
            und_all += und
            entries += info["evaluations"] * len(s)
            for cond, ok in zip(info["conds"], info["determined"]):
                assert ok or fit == 0.0, (k, "an estimate with correspondences is determined")
                if ok:
                    worst = max(worst, cond)
                    assert cond <= 1e4, (k, constrained, len(s), len(d), cond)
    print("worst scaled condition number %.3g; %d of %d entries undecided" % (worst, und_all, entries))
    assert und_all <= P.REF_CAP * entries
