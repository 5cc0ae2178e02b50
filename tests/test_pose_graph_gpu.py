"""GPU: multiway registration (alignnet_pose_graph_optimize, csrc/alignnet_posegraph.hip) against the restatement tests/pose_graph_ref.py, in both
forms (yaw + translation, full rotation): the linearisation through the debug hook, whole Levenberg-Marquardt runs, size edges, both placements of the
band (LDS / workspace), batches, chunks and input errors.

Bars.
System stage (debug_pose_graph_system against pose_graph_ref.system at the same poses), from fp64 rounding of the stated expressions, u = 2^-53:
  angles   64 u: the entries of D's rotation are two 3 x 3 products of entries <= 1 (<= 6 roundings of terms <= 1 each), atan2 / asin add a few ulp and
           have slope <= 1 / (R00^2 + R10^2) ~ 1;
  t        64 u S, S = |t_i| + |t_j| + |t_T| + 2 |c| (residual_scale): t is a sum of about a dozen terms, each at most S;
  chi2     2 dr^T |L| |r| + dr^T |L| dr + 64 u |r|^T |L| |r| with dr the two bars above (propagation + the rounding of the form itself);
  l        |dl / dchi2| = 2 mu^2 / (mu + chi2)^3 times chi2's bar, + 8 u;   F: sum of l times chi2's bar + 64 m u sum f;
  H, b     with the DEVICE's l (l is held to its own bar above): within 64 k u of the sum of the entry's terms' magnitudes, k = the edges that touch
           the entry; magnitudes l |J|^T |L| |J| and l |J|^T |L| rbar with the lever arm a and the residual replaced by the magnitudes of the terms
           they are differences of (pose_graph_ref.jac_magnitude, rbar >= (1, 1, 1, S, S, S)).
Whole runs (the restatement's decided runs): status and solves equal; pose entries within 64 x SELF_DIFF, floored at 1e-12 x max(1, extent) and
scaled by extent / EXTENT for graphs further out than the committed set.  SELF_DIFF is the restatement against itself with the edge list reversed
(another summation order of a correct fp64 implementation), the largest over the committed runs: 1.2e-13 measured, 1.5e-13 committed
(tests/test_pose_graph_cpu.py holds the measurement to it).  The device's worst difference to the restatement over the committed runs, measured on an
MI355X: 7.1e-15 (printed by test_whole_runs)."""
import numpy as np
import pytest

import alignnet3d
from tests import pose_graph_ref as G
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
U = G.U64


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs():
    """The committed runs, once: (graph, planted, restatement's result)."""
    out = []
    for k, (n, w, seed, c) in enumerate(G.RUNS):
        g, _, planted = G.run_graph(k)
        out.append((g, planted, G.optimize(g, constrained=c, threshold=G.MU_THRESHOLD)))
    return out


def pose_bar(g):
    return max(64 * G.SELF_DIFF * max(1.0, G.extent(g) / G.EXTENT), 1e-12 * G.extent(g))


def same(a, b):
    assert a["status"] == b["status"] and a["solves"] == b["solves"] and a["before"] == b["before"] and a["after"] == b["after"]
    for k in ("poses", "chi2", "weights", "pruned"):
        assert np.array_equal(a[k], b[k]), k


def against_ref(out, ref, g, what=""):
    assert out["status"] == G.STATUS[ref["status"]], (what, out["status"], G.STATUS[ref["status"]])
    worst = np.abs(out["poses"] - ref["poses"]).max() if len(out["poses"]) else 0.0
    if ref["margin"] >= G.UNDECIDED:
        assert out["solves"] == ref["solves"], (what, out["solves"], ref["solves"])
        assert worst <= pose_bar(g), (what, worst, pose_bar(g))
        assert np.array_equal(out["pruned"], ref["pruned"]), what
    return worst


def check_system(eng, g, c, mu):
    full = not c
    d = eng.debug_pose_graph_system(g, constrained=c, mu=mu)
    S = G.system(g, g["poses"], mu, full)
    m = len(g["i"])
    worst = {}
    bar_r = np.zeros((m, 6))
    for e in range(m):
        bar_r[e, :3] = 64 * U
        bar_r[e, 3:] = 64 * U * G.residual_scale(g["poses"][g["i"][e]], g["poses"][g["j"][e]], g["T"][e], g["c"][e])
    bar_r = bar_r if full else bar_r[:, 2:]
    assert np.all(np.abs(d["r"] - S["r"]) <= bar_r), np.abs(d["r"] - S["r"]).max()
    worst["r"] = (np.abs(d["r"] - S["r"]) / bar_r).max() if m else 0.0
    bar_chi2 = np.zeros(m)
    for e in range(m):
        L, r = np.abs(G.cut(g["info"][e], full)), np.abs(S["r"][e])
        bar_chi2[e] = 2 * bar_r[e] @ L @ r + bar_r[e] @ L @ bar_r[e] + 64 * U * (r @ L @ r)
    assert np.all(np.abs(d["chi2"] - S["chi2"]) <= bar_chi2), (np.abs(d["chi2"] - S["chi2"]) / bar_chi2).max()
    bar_l = 2 * mu * mu / (mu + S["chi2"]) ** 3 * bar_chi2 + 8 * U
    assert np.all(np.abs(d["weights"] - S["l"]) <= bar_l) and np.all(d["weights"][~g["uncertain"]] == 1.0)
    f = np.where(g["uncertain"], mu * S["chi2"] / (mu + S["chi2"]), S["chi2"])
    assert abs(d["F"] - S["F"]) <= (S["l"] * bar_chi2).sum() + 64 * m * U * f.sum()
    W = G.system(g, g["poses"], mu, full, weights=d["weights"])          # the same terms with the device's weights
    for key, cnt, mag in (("H", "cnt_H", "mag_H"), ("b", "cnt_b", "mag_b")):
        bar = 64 * W[cnt] * U * W[mag]
        diff = np.abs(d[key] - W[key])
        assert np.all(diff <= bar), (key, (diff / np.maximum(bar, 1e-300)).max())
        assert np.all(d[key][W[cnt] == 0] == 0.0)                          # entries no edge touches are exactly zero
        worst[key] = (diff[bar > 0] / bar[bar > 0]).max() if (bar > 0).any() else 0.0
    assert np.array_equal(d["H"], d["H"].T)
    return worst


# ---- the system stage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [True, False])
@pytest.mark.parametrize("n,w,seed", [(2, 1, 3), (5, 4, 4), (12, 4, 5), (25, 24, 6)])
def test_system_stage(eng, n, w, seed, c):
    g, _, _ = G.track(n, w, seed, constrained=c, wrong=min(3, max(0, n - 4)))
    worst = check_system(eng, g, c, G.default_mu(g, 1.0, G.MU_THRESHOLD))
    print("system stage, worst share of the bars:", {k: "%.3f" % v for k, v in worst.items()})


@pytest.mark.parametrize("c", [True, False])
def test_system_stage_repeated_edges_untied_nodes_far_frames(eng, c):
    g, _, _ = G.track(7, 3, 9, constrained=c, wrong=1, origin=(4000.0, -3000.0, 10.0))
    h, _, _ = G.track(3, 2, 10, constrained=c, wrong=0, origin=(4000.0, -3000.0, 10.0))
    rep = np.array([0, 4, 4, 7])                                             # edges given twice, one of them three times
    cat = lambda k, hk: np.concatenate([g[k], g[k][rep], hk])
    both = G.make_graph(np.concatenate([g["poses"], G.pose(1.0, [4000.0, -3001.0, 0.0])[None], h["poses"]]), cat("i", h["i"] + 8), cat("j", h["j"] + 8),
                        cat("T", h["T"]), cat("info", h["info"]), cat("c", h["c"]), cat("uncertain", h["uncertain"]))
    assert G.tied(both).sum() == 7
    check_system(eng, both, c, 0.4)


# ---- whole runs -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [True, False])
def test_whole_runs(eng, refs, c):
    """The committed runs of one form in one call: chains of 12 and 40 nodes with windows 3 and 4, 17 and 18 nodes (64 and 68 unknowns), 25 nodes fully
    connected, 2, 3 and 30 nodes; three planted wrong edges from 12 nodes on."""
    pick = [k for k, r in enumerate(G.RUNS) if r[3] == c]
    outs = eng.pose_graph_optimize([refs[k][0] for k in pick], constrained=c, threshold=G.MU_THRESHOLD)
    worst, decided = 0.0, 0
    for k, out in zip(pick, outs):
        g, planted, ref = refs[k]
        assert out["mu"] == ref["mu"]
        worst = max(worst, against_ref(out, ref, g, G.RUNS[k]))
        decided += ref["margin"] >= G.UNDECIDED
        assert np.array_equal(out["pruned"], planted), G.RUNS[k]
        # (a single edge is met exactly from the start: its F is rounding, residuals of ~1e-16 squared times an information of ~1e3 -- the floor)
        assert abs(out["after"] - ref["after"]) <= 1e-9 * ref["before"] + 1e-24 and out["before"] >= out["after"]
    print("whole runs: worst pose difference %.3g (bar %.3g), %d of %d decided" % (worst, 64 * G.SELF_DIFF, decided, len(pick)))
    assert decided >= len(pick) - 1


@pytest.mark.parametrize("c", [True, False])
def test_size_edges(eng, c):
    """One node; two nodes with one edge given as (0, 1) and as (1, 0); two identical edges; a node without edges; a component that no edge joins
    to node 0 (it keeps its poses to the bit)."""
    one = G.make_graph([G.pose(0.2, [1.0, 2.0, 3.0])], [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), np.zeros((0, 3)), [])
    two, _, _ = G.track(2, 1, 21, constrained=c)
    back = G.make_graph(two["poses"], two["j"], two["i"], [G.inverse(two["T"][0])], two["info"], [(two["T"][0][:3, :3].T @ (two["c"][0] - two["T"][0][:3, 3]))],
                        two["uncertain"])
    dup = G.make_graph(two["poses"], [0, 0], [1, 1], [two["T"][0]] * 2, [two["info"][0]] * 2, [two["c"][0]] * 2, [False, True])
    g, _, _ = G.track(5, 2, 22, constrained=c, wrong=0)
    h, _, _ = G.track(4, 3, 23, constrained=c, wrong=0, rot_noise=2e-2, shift_noise=5e-2)
    lone = G.make_graph(np.concatenate([g["poses"], G.pose(0.3, [5.0, 1.0, 0.0])[None]]), g["i"], g["j"], g["T"], g["info"], g["c"], g["uncertain"])
    poses = np.concatenate([g["poses"], h["poses"]])
    parts = G.make_graph(poses, np.concatenate([g["i"], h["i"] + 5]), np.concatenate([g["j"], h["j"] + 5]), np.concatenate([g["T"], h["T"]]),
                         np.concatenate([g["info"], h["info"]]), np.concatenate([g["c"], h["c"]]), np.concatenate([g["uncertain"], h["uncertain"]]))
    graphs = [one, two, back, dup, lone, parts]
    mu = 0.5
    outs = eng.pose_graph_optimize(graphs, constrained=c, mu=mu)
    for name, gr, out in zip("one two back dup lone parts".split(), graphs, outs):
        ref = G.optimize(gr, mu=mu, constrained=c)
        against_ref(out, ref, gr, name)
        same(out, eng.pose_graph_optimize([gr], constrained=c, mu=mu)[0])
    assert outs[0]["status"] == "EMPTY" and outs[0]["solves"] == 0 and np.array_equal(outs[0]["poses"], one["poses"])
    assert np.array_equal(outs[4]["poses"][5], lone["poses"][5]) and not np.array_equal(outs[4]["poses"][1:5], lone["poses"][1:5])
    assert np.array_equal(outs[5]["poses"][5:], poses[5:]) and np.all(outs[5]["chi2"][len(g["i"]):] > 0)
    assert outs[3]["weights"][0] == 1.0 and 0.99 < outs[3]["weights"][1] <= 1.0   # (the pair is met exactly: chi2 is rounding)
    # every node untied but node 0 (no edge reaches it): nothing to move
    adrift = G.make_graph(poses[4:], h["i"] + 1, h["j"] + 1, h["T"], h["info"], h["c"], h["uncertain"])
    out = eng.pose_graph_optimize([adrift], constrained=c, mu=mu)[0]
    assert out["status"] == "EMPTY" and np.array_equal(out["poses"], poses[4:]) and out["before"] == out["after"] > 0


def test_far_frames(eng):
    """A track whose frames lie 5 km from the origin, centres at the crops' means: the bars relative to the extent."""
    for c, seed in ((True, 41), (False, 46)):
        g, _, planted = G.track(14, 4, seed, constrained=c, origin=(3000.0, -4000.0, 20.0))
        assert G.extent(g) > 3900
        ref = G.optimize(g, constrained=c, threshold=G.MU_THRESHOLD)
        assert ref["margin"] >= G.UNDECIDED, "pick another seed on the CPU"
        out = eng.pose_graph_optimize([g], constrained=c, threshold=G.MU_THRESHOLD)[0]
        worst = against_ref(out, ref, g, "far")
        print("far frames: worst pose difference %.3g (bar %.3g)" % (worst, pose_bar(g)))
        assert np.array_equal(out["pruned"], planted)


def test_all_uncertain_graph(eng):
    for c, seed in ((True, 53), (False, 52)):
        g, _, planted = G.track(10, 3, seed, constrained=c, all_uncertain=True, wrong=2)
        ref = G.optimize(g, constrained=c, threshold=G.MU_THRESHOLD)
        assert ref["margin"] >= G.UNDECIDED, "pick another seed on the CPU"
        out = eng.pose_graph_optimize([g], constrained=c, threshold=G.MU_THRESHOLD)[0]
        against_ref(out, ref, g, "all uncertain")
        assert np.all(out["weights"] < 1.0) and np.array_equal(out["pruned"], planted)


# ---- placements, batches, chunks -----------------------------------------------------------------------------------------------------------------
def test_band_in_lds_and_in_the_workspace_give_the_same_bits(eng, refs):
    """The region of a z-constrained chain with window 4 is 42 N doubles, N = 4 (n - 1): 120 nodes (19,992) lie just below the LDS budget of 20,000,
    121 nodes (20,160) just above.  Both are also run with every band forced into the workspace; and so are the small committed runs."""
    big = [G.track(n, 4, 60 + n, wrong=3)[0] for n in (120, 121)]
    small = [refs[k][0] for k, r in enumerate(G.RUNS) if r[3]]
    try:
        eng.set_option("pose_graph_lds_budget", -1)
        a = eng.pose_graph_optimize(big, threshold=G.MU_THRESHOLD)
        assert eng.get_option("pose_graph_lds_graphs") == 1
        eng.pose_graph_optimize(big[:1], threshold=G.MU_THRESHOLD)
        assert eng.get_option("pose_graph_lds_graphs") == 1
        eng.pose_graph_optimize(big[1:], threshold=G.MU_THRESHOLD)
        assert eng.get_option("pose_graph_lds_graphs") == 0
        sa = eng.pose_graph_optimize(small, threshold=G.MU_THRESHOLD)
        assert eng.get_option("pose_graph_lds_graphs") == len(small)
        eng.set_option("pose_graph_lds_budget", 0)
        b = eng.pose_graph_optimize(big, threshold=G.MU_THRESHOLD)
        sb = eng.pose_graph_optimize(small, threshold=G.MU_THRESHOLD)
        assert eng.get_option("pose_graph_lds_graphs") == 0
    finally:
        eng.set_option("pose_graph_lds_budget", -1)
    for x, y in zip(a + sa, b + sb):
        same(x, y)
    for out in a:
        assert out["status"] == "CONVERGED" and out["after"] < out["before"] and out["pruned"].sum() == 3


def _forty(c):
    """40 heterogeneous graphs, empty ones among them."""
    graphs = []
    for k in range(40):
        n = (1, 2, 3, 5, 9, 12, 17, 18, 26, 33)[k % 10]
        if n == 1:
            graphs.append(G.make_graph([G.pose(0.1 * k, [k, 0.0, 0.0])], [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), np.zeros((0, 3)), []))
            continue
        g, _, _ = G.track(n, 1 + k % 5, 700 + k, constrained=c, wrong=k % 3 if n > 5 else 0, all_uncertain=k % 7 == 0)
        if k % 10 == 2:   # nodes and no edges
            g = G.make_graph(g["poses"], [], [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), np.zeros((0, 3)), [])
        graphs.append(g)
    return graphs


@pytest.mark.parametrize("c", [True, False])
def test_forty_graphs_in_one_call_and_in_chunks(eng, c):
    graphs = _forty(c)
    try:
        eng.set_option("pose_graph_ws_budget", 0)
        batch = eng.pose_graph_optimize(graphs, constrained=c, threshold=G.MU_THRESHOLD)
        assert eng.get_option("pose_graph_chunks") == 1
        for g, out in zip(graphs, batch):
            same(out, eng.pose_graph_optimize([g], constrained=c, threshold=G.MU_THRESHOLD)[0])
        assert sum(o["status"] == "EMPTY" for o in batch) == 8
        for g, o in zip(graphs, batch):
            if len(g["i"]):   # (a run that ends on rounding -- the restatement's undecided runs -- may stop as STALLED: fourteen rejections in a row)
                assert o["status"] in ("CONVERGED", "STALLED") and o["after"] <= o["before"], (len(g["poses"]), o["status"])
        assert sum(o["status"] == "CONVERGED" for o in batch) >= 28
        eng.set_option("pose_graph_ws_budget", 64 << 10)
        chunked = eng.pose_graph_optimize(graphs, constrained=c, threshold=G.MU_THRESHOLD)
        chunks = eng.get_option("pose_graph_chunks")
        assert 3 <= chunks <= 40, chunks
        eng.set_option("pose_graph_lds_budget", 0)                      # and with the bands in the chunks' workspace
        chunked_ws = eng.pose_graph_optimize(graphs, constrained=c, threshold=G.MU_THRESHOLD)
        assert eng.get_option("pose_graph_chunks") > chunks
    finally:
        eng.set_option("pose_graph_ws_budget", 0)
        eng.set_option("pose_graph_lds_budget", -1)
    for x, y, z in zip(batch, chunked, chunked_ws):
        same(x, y)
        same(x, z)


def test_max_solves_and_timer(eng, refs):
    g, _, ref = refs[0]
    out = eng.pose_graph_optimize([g], threshold=G.MU_THRESHOLD, max_solves=2)[0]
    assert out["status"] == "ITERATIONS" and out["solves"] == 2 and out["after"] < out["before"]
    eng.profile_enable(True)
    try:
        eng.profile_read(reset=True)
        eng.pose_graph_optimize([g, g], threshold=G.MU_THRESHOLD)
        k = eng.profile_kernels()
        assert k["pose_graph"][1] == 1 and k["pose_graph"][0] > 0
    finally:
        eng.profile_read(reset=True)
        eng.profile_enable(False)


def test_bad_input_raises_before_the_device(eng, refs):
    g, _, _ = refs[0]
    before = eng.pose_graph_optimize([g], threshold=G.MU_THRESHOLD)[0]

    def broken(**kw):
        h = {k: np.array(v) for k, v in g.items()}
        for k, (idx, v) in kw.items():
            h[k][idx] = v
        return h
    for bad in (broken(i=(3, 12)), broken(j=(0, -1)), broken(i=(5, int(g["j"][5]))), broken(T=((2, 1, 3), np.nan)), broken(info=((1, 0, 4), np.inf)),
                broken(poses=((3, 0, 0), np.nan)), broken(c=((0, 1), np.inf))):
        with pytest.raises(ValueError):
            eng.pose_graph_optimize([g, bad], threshold=G.MU_THRESHOLD)
    for mu in (0.0, -1.0, np.nan):
        with pytest.raises(ValueError):
            eng.pose_graph_optimize([g], mu=mu)
    with pytest.raises(ValueError):
        eng.pose_graph_optimize([g], max_solves=0)
    same(before, eng.pose_graph_optimize([g], threshold=G.MU_THRESHOLD)[0])


def test_library_checks_its_arguments_itself(eng, refs):
    """The C entry point, past the Python checks: an index out of range, i == j, a non-finite entry and mu <= 0 are errors of the call."""
    import ctypes as C
    g, _, _ = refs[0]
    node_off, edge_off, poses, edges, T, info, c, unc = eng._pose_graph_arrays([g])
    dp, ip, lp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))
    out = np.empty_like(poses)

    def call(edges=edges, T=T, mu=1.0, max_solves=100):
        m = np.array([mu])
        return eng._lib.alignnet_pose_graph_optimize(eng._h, 1, lp(node_off), lp(edge_off), dp(poses), ip(edges), dp(T), dp(info), dp(c), ip(unc), dp(m), 0, max_solves,
                                                     dp(out), None, None, None, None, None, None)
    assert call() == 0
    e1, e2, T2 = edges.copy(), edges.copy(), T.copy()
    e1[2, 0], e2[2, 0], T2[1, 0, 3] = 12, e2[2, 1], np.inf
    for kw, word in ((dict(edges=e1), "out of range"), (dict(edges=e2), "itself"), (dict(T=T2), "finite"), (dict(mu=0.0), "mu"), (dict(max_solves=0), "max_solves")):
        assert call(**kw) != 0
        assert word in eng._lib.alignnet_last_error(eng._h).decode(), kw
    assert call() == 0
