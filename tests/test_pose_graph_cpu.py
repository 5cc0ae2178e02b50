"""CPU: multiway registration -- the surface of alignnet_pose_graph_optimize / Engine.pose_graph_optimize, the restatement tests/pose_graph_ref.py on
its own (Jacobians against differences, monotone objective, planted outliers = pruned, the cap on undecided runs, held nodes) and
alignnet3d.tracks.build_graphs on hand-made pairs.  No GPU."""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

import alignnet3d
from alignnet3d import _capi, tracks
from tests import pose_graph_ref as G
from tests.icp_plane_ref import rigid_about

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alignnet_pose_graph_optimize", "alignnet_debug_pose_graph_system")


def test_symbols_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alignnet_hip.h")).read(), flags=re.S)
    lib = alignnet3d.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _capi.SYMBOLS and hasattr(lib, name), name
    assert lib.alignnet_abi_version() == 1
    for k, name in enumerate(alignnet3d.Engine.POSE_GRAPH_STATUS):
        assert re.search(r"#define ALIGNNET_POSE_GRAPH_%s %d\b" % (name, k), hdr), name
    assert alignnet3d.Engine.POSE_GRAPH_STATUS == G.STATUS and alignnet3d.Engine.POSE_GRAPH_PRUNE == G.PRUNE


def test_engine_wrappers_exist():
    import inspect
    sig = inspect.signature(alignnet3d.Engine.pose_graph_optimize)
    assert [(k, p.default) for k, p in sig.parameters.items()][2:] == [("constrained", True), ("mu", None), ("preference", 1.0), ("threshold", 0.02),
                                                                      ("max_solves", 100)]
    assert callable(alignnet3d.Engine.debug_pose_graph_system)
    assert "pose_graph" in alignnet3d.Engine.PROFILED_KERNELS
    assert "alignnet_posegraph.hip" in open(os.path.join(ROOT, "alignnet-3d_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("full", [False, True])
def test_jacobians_match_central_differences(full):
    """At poses whose D is within 1e-3 of the identity.  The analytic Jacobian is the first-order one AT D = I.  A step s moves D to (I + [s]) D with [s]
    the small motion A s (|A| <= arm = 1 + |a|, a the lever arm of the edge); the residual of (I + [s]) (I + E), |E| <= eps = 1e-3, is
    r(E) + A s + (cross term <= 2 |A s| |E| arm-free part + second order of s <= |A s|^2 arm): per unit step the difference to A is at most
    4 arm eps (cross term, with room for the angles' own second order) + arm h^2 (what a central difference leaves of the step's higher orders) +
    64 u S / h (rounding of the difference, S the scale of the terms t is a sum of), with h = 1e-5.  The entries of A are 1 (rotations) and up
    to |a| ~ 10 (lever arms): a wrong sign, a transposed rotation or a swapped role misses the bar by one to two orders of magnitude."""
    rng = np.random.default_rng(11 + full)
    d, h, eps = G.dim(full), 1e-5, 1e-3
    for trial in range(20):
        z = [0, 0, 1] if not full else [1, 1, 1]
        Xi = rigid_about(np.zeros(3), rng.uniform(-3, 3, 3) * z, rng.uniform(-5, 5, 3))
        Xj = rigid_about(np.zeros(3), rng.uniform(-3, 3, 3) * z, rng.uniform(-5, 5, 3))
        c = rng.uniform(-3, 3, 3)
        E = rigid_about(c, rng.uniform(-1, 1, 3) * z * eps / 16, rng.uniform(-1, 1, 3) * eps / 4)      # D = E: within eps of the identity
        T = G.inverse(E) @ G.inverse(Xj) @ Xi
        D = G.inverse(Xj) @ Xi @ G.inverse(T)
        assert np.abs(D - np.eye(4)).max() <= eps
        Ji, Jj = G.jac(Xj, Xi[:3, 3], c, full), -G.jac(Xj, Xj[:3, 3], c, full)
        arm = 1.0 + max(np.linalg.norm(c - (G.inverse(Xj) @ Xi)[:3, 3]), np.linalg.norm(c))
        bar = 4 * arm * eps + arm * h * h + 64 * G.U64 * G.residual_scale(Xi, Xj, T, c) / h
        for which, J in ((0, Ji), (1, Jj)):
            for q in range(d):
                x = np.zeros(d); x[q] = h
                def moved(s):
                    P = G.apply_step(np.stack([np.eye(4), Xi if which == 0 else Xj]), s * x, full)[1]
                    return G.residual(P if which == 0 else Xi, Xj if which == 0 else P, T, c, full)
                num = (moved(1.0) - moved(-1.0)) / (2 * h)
                assert np.abs(num - J[:, q]).max() <= bar, (trial, which, q, np.abs(num - J[:, q]).max(), bar)
                assert np.abs(J[:, q]).max() >= 0.5 > 4 * bar      # (every column has an entry the bar resolves)


@pytest.fixture(scope="module")
def runs():
    out = []
    for k, (n, w, seed, c) in enumerate(G.RUNS):
        g, truth, planted = G.run_graph(k)
        info = {}
        out.append((g, truth, planted, G.optimize(g, constrained=c, threshold=G.MU_THRESHOLD, info=info), info))
    return out


def test_objective_never_rises_over_accepted_steps(runs):
    for g, _, _, res, info in runs:
        tr = np.array(info["F_trace"])
        assert len(tr) >= 2 and np.all(np.diff(tr) <= 0) and tr[0] == res["before"] and tr[-1] == res["after"]
        assert res["status"] == 0 and res["solves"] >= len(tr) - 1


def test_planted_outliers_are_the_pruned_edges(runs):
    for (n, w, seed, c), (g, _, planted, res, _) in zip(G.RUNS, runs):
        assert np.array_equal(res["pruned"], planted), (n, w, seed, c)
        assert planted.sum() == (3 if n >= 12 else 0)
        assert np.all(res["weights"][~g["uncertain"]] == 1.0)


def test_optimised_tracks_are_closer_to_the_truth_where_the_window_is_wide(runs):
    for (n, w, seed, c), (g, truth, _, res, _) in zip(G.RUNS, runs):
        if w >= 24:
            err = lambda X: np.abs(X[:, :3, 3] - truth[:, :3, 3]).max()
            assert err(res["poses"]) < 0.25 * err(g["poses"]), (err(res["poses"]), err(g["poses"]))


def test_cap_on_undecided_runs(runs):
    undecided = [res["margin"] < G.UNDECIDED for _, _, _, res, _ in runs]
    assert sum(undecided) <= G.CAP * len(runs), undecided


def test_self_difference_with_the_edge_list_reversed(runs):
    """The yardstick of the device's bar: another summation order of the same fp64 computation.  Decided runs take the same decisions either way."""
    worst, ext = 0.0, 0.0
    for (n, w, seed, c), (g, _, _, res, _) in zip(G.RUNS, runs):
        rev = G.optimize(G.reversed_edges(g), constrained=c, threshold=G.MU_THRESHOLD)
        ext = max(ext, G.extent(g))
        if min(res["margin"], rev["margin"]) >= G.UNDECIDED:
            assert rev["solves"] == res["solves"] and rev["status"] == res["status"]
            worst = max(worst, np.abs(rev["poses"] - res["poses"]).max())
            assert np.array_equal(rev["pruned"][::-1], res["pruned"])
    print("self-difference %.3g, extent %.3g" % (worst, ext))
    assert G.SELF_DIFF / 8 <= worst <= G.SELF_DIFF and G.EXTENT / 2 <= ext <= G.EXTENT


def test_untied_nodes_keep_their_pose_to_the_bit():
    """A node without edges and a component that no edge joins to node 0: zero gradient rows, zero step, the given pose to the bit; the tied part is
    optimised as if the others were not there."""
    for c in (True, False):
        g, _, _ = G.track(6, 2, 31, constrained=c, wrong=0)
        h, _, _ = G.track(4, 2, 32, constrained=c, wrong=0, rot_noise=2e-2, shift_noise=5e-2)     # its edges disagree: left alone it would move
        n = 6 + 1 + 4
        poses = np.concatenate([g["poses"], G.pose(0.3, [5.0, 1.0, 0.0])[None], h["poses"]])
        both = G.make_graph(poses, np.concatenate([g["i"], h["i"] + 7]), np.concatenate([g["j"], h["j"] + 7]), np.concatenate([g["T"], h["T"]]),
                            np.concatenate([g["info"], h["info"]]), np.concatenate([g["c"], h["c"]]), np.concatenate([g["uncertain"], h["uncertain"]]))
        assert G.tied(both).tolist() == [True] * 6 + [False] * 5
        mu = 0.3
        S = G.system(both, both["poses"], mu, not c)
        d = G.dim(not c)
        assert np.all(S["b"][d * 5:] == 0) and np.all(S["H"][d * 5:] == 0) and np.all(S["H"][:, d * 5:] == 0)
        res, alone = G.optimize(both, mu=mu, constrained=c), G.optimize(g, mu=mu, constrained=c)
        assert np.array_equal(res["poses"][6:], poses[6:]) and n == len(res["poses"])
        # the tied part reaches the minimum it reaches alone (F carries the held edges' constant, so the stop test may fall a step apart: both
        # stop once a step gains less than 1e-12 F, which leaves the poses within ~1e-6 of the minimum)
        assert np.abs(res["poses"][:6] - alone["poses"]).max() < 1e-6
        assert res["after"] > alone["after"] and np.all(res["chi2"][len(g["i"]):] > 0)          # the held component's edges still count in F


def test_empty_graphs_and_bad_mu():
    one = G.make_graph([np.eye(4)], [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), np.zeros((0, 3)), [])
    res = G.optimize(one)
    assert G.STATUS[res["status"]] == "EMPTY" and res["solves"] == 0 and res["before"] == res["after"] == 0.0
    g, _, _ = G.track(3, 2, 5)
    with pytest.raises(ValueError):
        G.optimize(g, mu=0.0)
    with pytest.raises(ValueError):
        alignnet3d.Engine._pose_graph_mu([g], g["info"], np.array([0, 3]), -1.0, 1.0, 0.02)
    assert alignnet3d.Engine._pose_graph_mu([g], g["info"], np.array([0, 3]), None, 1.0, 0.05)[0] == G.default_mu(g, 1.0, 0.05)


# ---- tracks.build_graphs ------------------------------------------------------------------------------------------------------------------------
P = namedtuple("P", "seq frames track timestamps")


def _yaw(a, t):
    return G.pose(a, t)


def test_build_graphs_on_hand_made_pairs():
    # track 7 of sequence 2 is seen in frames 3, 4, 5 and, after a hole at 6, in 7, 8; track 1 of sequence 0 in frames 0, 1; track 9 of sequence 2 in
    # frames 0 and 2 only (no consecutive frames: no graph)
    stamp = lambda f: 0.1 * f
    mk = lambda seq, track, f, s: P(seq, (f, f + s), track, (stamp(f), stamp(f + s)))
    pairs = [mk(2, 7, 3, 1), mk(2, 7, 4, 1), mk(2, 7, 7, 1), mk(0, 1, 0, 1), mk(2, 7, 3, 2), mk(2, 7, 5, 2), mk(2, 7, 4, 3), mk(2, 7, 3, 4), mk(2, 9, 0, 2)]
    rng = np.random.default_rng(2)
    Ts = np.stack([_yaw(rng.uniform(-0.2, 0.2), rng.uniform(-1, 1, 3)) for _ in pairs])
    Ls = rng.uniform(0, 1, (len(pairs), 6, 6))
    cs = rng.uniform(-1, 1, (len(pairs), 3))
    gs = tracks.build_graphs(pairs, Ts, Ls, cs, max_skip=3)
    assert [(g["seq"], g["track"], g["frames"].tolist()) for g in gs] == [(0, 1, [0, 1]), (2, 7, [3, 4, 5]), (2, 7, [7, 8])]
    a, b, c = gs
    # the hole splits the track; the gap-2 pair (5, 7) and the gap-3 pair (4, 7) cross it and are dropped; the gap-4 pair is beyond max_skip
    assert b["pair_index"].tolist() == [0, 1, 4] and c["pair_index"].tolist() == [2] and a["pair_index"].tolist() == [3]
    assert b["i"].tolist() == [0, 1, 0] and b["j"].tolist() == [1, 2, 2] and b["uncertain"].tolist() == [False, False, True]
    assert np.array_equal(b["T"], Ts[[0, 1, 4]]) and np.array_equal(b["info"], Ls[[0, 1, 4]]) and np.array_equal(b["c"], cs[[0, 1, 4]])
    assert np.allclose(b["timestamps"], [0.3, 0.4, 0.5]) and np.allclose(c["timestamps"], [0.7, 0.8])
    # chained poses: X_0 = I, X_{k+1} = X_k T_{k,k+1}^-1
    assert np.array_equal(b["poses"][0], np.eye(4))
    assert np.allclose(b["poses"][1], np.linalg.inv(Ts[0]), atol=1e-14) and np.allclose(b["poses"][2], np.linalg.inv(Ts[0]) @ np.linalg.inv(Ts[1]), atol=1e-14)
    assert np.allclose(c["poses"][1] @ Ts[2], np.eye(4), atol=1e-14)
    # with max_skip 1 only the odometry is left; the graphs feed the restatement as they are
    assert [g["uncertain"].tolist() for g in tracks.build_graphs(pairs, Ts, Ls, cs, max_skip=1)] == [[False], [False, False], [False]]
    res = G.optimize(b, mu=1.0)
    assert res["poses"].shape == (3, 4, 4)
    with pytest.raises(ValueError):
        tracks.build_graphs(pairs, Ts[:-1], Ls, cs, 3)
    # speeds: a pose that maps frame k onto frame 0 by a shift of -k along x puts the object k further along x
    X = np.stack([_yaw(0.0, [-1.5 * k, 0.0, 0.0]) for k in range(4)])
    assert np.allclose(tracks.speeds(X, [0.0, 0.1, 0.2, 0.4], [10.0, 2.0, 0.0]), [15.0, 15.0, 7.5])
