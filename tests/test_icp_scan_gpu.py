"""GPU: the ICP kernel's nearest-neighbour scan under load (csrc/alignnet_icp.hip: one fp32 pass per lane, an error bound choosing none / single /
walk per lane, the fp64 tail behind the LDS stage, the quad's merge) against the fp64 restatement with margins of tests/icp_scan_ref.py, on inputs
built to break an fp32 certificate: dense clouds up to 4 km from the origin (a plain float32 argmin is wrong for 1 - 5 % of their points), planted
near-ties below what fp32 resolves placed inside one lane's slice, across slices and across the LDS / tail border, exact radius edges, the launch
geometry's size edges, the estimate's branches.  Per point through the read-back of ONE evaluation (Engine.debug_icp_scan: the shipped scan source
compiled with a record behind it), so that one flipped decision cannot hide in a sum; whole runs to the bars of tests/test_icp_gpu.py.

A source point whose fp64 margin is below UNDECIDED x b64 (tests/icp_scan_ref.py: how far two correct fp64 evaluations may differ) is undecided and
skipped; at most POINT_CAP of a test's points and one pair per whole-run test may be (tests/test_icp_scan_cpu.py: the restatement alone finds a tenth
of the first and none of the second on these seeds).  What is asked of the paths is what ANY sound certificate must do, so no number of the kernel
is used: a pair fp32 cannot resolve (gap < need32 / 8) inside one slice makes that lane walk, across slices leaves both lanes in play, a winner in
the tail is reported from the tail -- and a second target a thousand times farther than fp32 blurs must NOT make a lane walk."""

import numpy as np
import pytest

import alignnet3d
from tests import icp_full_ref as F
from tests import icp_scan_ref as S
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu

NONE, SINGLE, WALK = 0, 1, 2


def _engine():
    return alignnet3d.Engine(small_cfg(N=64, nb=12))


def _scan(eng, name, src, dst, T, radius, tally, lds_points=0, exact=False, rmse_tol=1e-12, full=True):
    """One evaluation, per point: the read-back against the restatement; the same evaluation through icp_refine(its=0).  Returns (restatement, read-back)."""
    e = S.evaluate_with_margins(src, dst, T, radius, exact=exact)
    d = eng.debug_icp_scan(src, dst, T, radius=radius, lds_points=lds_points)
    ok = ~e["undecided"]
    lanes = [int((d["lanes"] == c).sum()) for c in (NONE, SINGLE, WALK)]
    wrong32 = float(((S.fp32_argmin(src, dst, T) != e["index"]) & (e["gap"] > 0)).mean()) if len(src) else 0.0
    err = np.abs(d["dist2"] - e["best"])[ok]
    print("%s: %d points, %d undecided, lanes none / single / walk %d / %d / %d, tail winners %d, float32 argmin wrong %.2f %%, lds_points %d, "
          "worst distance error %.3g (%.3g of its bound)" % (name, len(src), (~ok).sum(), *lanes, d["tail_won"].sum(), 100 * wrong32, d["lds_points"],
                                                             err.max() if err.size else 0.0, (err / (S.UNDECIDED * S.b64(e["P64"], e["best"])[ok] + 1e-300)).max() if err.size else 0.0))
    tally[0] += int((~ok).sum()); tally[1] += len(src)
    assert d["lds_points"] == (lds_points or max(1, min(S.LDS_BUDGET, len(dst))))
    bad = np.flatnonzero(ok & (d["index"] != e["index"]))
    assert bad.size == 0, (name, "wrong target for decided points", bad[:8], d["index"][bad[:8]], e["index"][bad[:8]], d["lanes"][bad[:8]], e["gap"][bad[:8]])
    assert np.all(err == 0.0) if exact else np.all(err <= S.UNDECIDED * S.b64(e["P64"], e["best"])[ok]), name
    assert np.array_equal(d["inlier"][ok], e["inlier"][ok]), name
    assert np.array_equal(d["tail_won"], d["index"] >= d["lds_points"]), name
    if full:   # the full-rotation instantiation runs the same scan source (the compiler may contract its arithmetic differently: held to the restatement, not to bits)
        f = eng.debug_icp_scan(src, dst, T, radius=radius, lds_points=lds_points, constrained=False)
        ferr = np.abs(f["dist2"] - e["best"])[ok]
        assert np.array_equal(f["index"][ok], e["index"][ok]) and np.array_equal(f["inlier"][ok], e["inlier"][ok]), (name, "full rotation")
        assert np.all(ferr == 0.0) if exact else np.all(ferr <= S.UNDECIDED * S.b64(e["P64"], e["best"])[ok]), (name, "full rotation")
        assert np.array_equal(f["tail_won"], f["index"] >= f["lds_points"]) and f["lds_points"] == d["lds_points"]
        if ok.all():
            assert f["fitness"] == e["fitness"] and abs(f["rmse"] - e["rmse"]) < rmse_tol, (name, "full rotation")
    if lds_points == 0:   # the shipped instantiation on the same evaluation
        r = eng.icp_refine([src], [dst], [T], radius=radius, its=0)
        assert r["fitness"][0] == d["fitness"] and r["rmse"][0] == d["rmse"] and r["iterations"][0] == 0 and np.array_equal(r["transforms"][0], np.asarray(T, np.float64))
    if ok.all():
        assert d["fitness"] == e["fitness"] and abs(d["rmse"] - e["rmse"]) < rmse_tol, (name, d["fitness"], e["fitness"], d["rmse"] - e["rmse"])
    return e, d


@pytest.mark.parametrize("offset", S.OFFSETS)
def test_scan_per_point_dense_far_frames(gpu_required, offset):
    eng = _engine()
    tally = [0, 0]
    for shape, n2, off, gen in S.dense_cases():
        if off != offset:
            continue
        src, dst, T, _ = S.dense_pair(shape, n2, off, gen, S.DENSE_SEED)
        for radius in (0.02, 0.1):
            _scan(eng, "%s n2 %d offset %s general %d radius %.2f" % (shape, n2, off, gen, radius), src, dst, T, radius, tally,
                  rmse_tol=1e-12 if S.offset_norm(off) <= 50 else 1e-9)
        if n2 == 4000:   # the same cloud with a tail: 3000 targets staged, 1000 behind them
            _scan(eng, "%s n2 %d offset %s general %d lds 3000" % (shape, n2, off, gen), src, dst, T, 0.02, tally, lds_points=3000)
    assert tally[0] <= S.POINT_CAP * tally[1], tally
    eng.close()


@pytest.mark.parametrize("offset", [0.0, 50.0])
def test_scan_planted_near_ties_take_their_paths(gpu_required, offset):
    eng = _engine()
    tally = [0, 0]
    src, dst, T, plan = S.planted_pair(offset, seed=3)
    e, d = _scan(eng, "planted offset %s" % offset, src, dst, T, S.PLANT_RADIUS, tally, lds_points=S.PLANT_LDS)
    assert tally[0] == 0 and np.array_equal(d["index"], plan["near"])
    hard = plan["rclass"] != 0                      # gap < need32 / 8: no fp32 evaluation tells the two apart
    k = np.arange(len(src))
    near_lane, far_lane = d["lanes"][k, plan["near"] % 4], d["lanes"][k, plan["far"] % 4]
    cat = np.array(S.PLANT_CATEGORIES)[plan["category"]]
    sel = hard & (cat == "same_slice")
    assert sel.sum() >= 60 and np.all(near_lane[sel] == WALK), np.flatnonzero(sel & (near_lane != WALK))
    sel = hard & (cat == "cross_slice")
    assert sel.sum() >= 60 and np.all(near_lane[sel] != NONE) and np.all(far_lane[sel] != NONE)
    sel = (cat == "lds_tail") & (plan["near"] < S.PLANT_LDS)
    assert sel.sum() >= 32 and np.all(near_lane[sel] != NONE) and not d["tail_won"][sel].any()
    sel = plan["near"] >= S.PLANT_LDS
    assert sel.sum() >= 100 and d["tail_won"][sel].all()
    print("planted offset %s: lanes of the nearer target none / single / walk %s" % (offset, [int((near_lane == c).sum()) for c in (NONE, SINGLE, WALK)]))
    # the same cloud as shipped (everything LDS-resident): the tail categories become slice categories
    e, d = _scan(eng, "planted offset %s, no tail" % offset, src, dst, T, S.PLANT_RADIUS, tally)
    same = hard & (plan["near"] % 4 == plan["far"] % 4)
    assert same.sum() >= 60 and np.all(d["lanes"][k, plan["near"] % 4][same] == WALK) and not d["tail_won"].any()
    assert np.all(d["lanes"][k, plan["far"] % 4][hard] != NONE)
    eng.close()


@pytest.mark.parametrize("offset", [0.0, 50.0])
def test_scan_planted_three_and_four_way_near_ties(gpu_required, offset):
    """Three and four targets no fp32 evaluation can order: a lane keeps only its two smallest fp32 distances, so a slice holding all of them must be
    walked; spread over slices, every lane holding one stays in play and the quad's merge picks among three / four; with part of them in the tail the
    winner is reported from where it lies."""
    eng = _engine()
    tally = [0, 0]
    src, dst, T, plan = S.planted_multi(offset, seed=4)
    k = np.arange(len(src))
    for lds in (S.PLANT_LDS, 0):
        e, d = _scan(eng, "planted 3 / 4 offset %s lds %d" % (offset, lds), src, dst, T, S.PLANT_RADIUS, tally, lds_points=lds)
        L = d["lds_points"]
        assert tally[0] == 0 and np.array_equal(d["index"], plan["idx"][:, 0]) and d["inlier"].all()
        walks = 0
        for t in range(4):
            j = plan["idx"][:, t]
            held = (j >= 0) & (j < L)                                         # this planted target is LDS-resident: its lane cannot drop it
            assert np.all(d["lanes"][k, j % 4][held] != NONE), (lds, t)
        for m in (3, 4):
            same = (plan["m"] == m) & (plan["layout"] == 0)
            assert same.sum() >= 32 and np.all(d["lanes"][k, plan["idx"][:, 0] % 4][same] == WALK), (lds, m)
            spread = (plan["m"] == m) & (plan["layout"] == 1)
            assert spread.sum() >= 32 and np.all((d["lanes"][spread] != NONE).sum(1) >= m), (lds, m)
            walks += int((d["lanes"][same] == WALK).sum())
        assert np.array_equal(d["tail_won"], plan["idx"][:, 0] >= L)
        print("planted 3 / 4 offset %s lds %d: %d tail winners, %d walking lanes on the same-slice sets" % (offset, L, d["tail_won"].sum(), walks))
    assert (plan["idx"][:, 0] >= S.PLANT_LDS).sum() >= 16
    eng.close()


def test_scan_certificate_stays_useful(gpu_required):
    """On points whose second target is farther than the nearest by more than 1000 x need32, no lane may walk: a threshold that degenerates into
    `always walk` is as correct as the all-fp64 scan and three times slower, and no output-only test sees it."""
    from tests.test_icp_gpu import _pairs
    eng = _engine()
    src, dst, inits, _ = _pairs(7, seed=2)
    tally = [0, 0]
    clear = walked = lanes = 0
    for k in range(7):
        e, d = _scan(eng, "uniform cloud %d" % k, src[k], dst[k], inits[k], 0.1, tally)
        sel = e["gap"] > 1000 * S.need32(e["P32"], e["second"])
        clear += int(sel.sum()); walked += int((d["lanes"][sel] == WALK).sum()); lanes += int((d["lanes"][sel] != NONE).sum())
    print("clear points %d of %d: %d lanes in play, %d walks" % (clear, tally[1], lanes, walked))
    assert clear >= 0.99 * tally[1] and walked == 0 and lanes >= clear
    eng.close()


def test_scan_radius_edge(gpu_required):
    eng = _engine()
    tally = [0, 0]
    for radius in (2.0 ** -4, 2.0 ** -3):
        src, dst, T, n_on = S.radius_edge_pair(radius)
        for lds in (0, 64):
            e, d = _scan(eng, "radius edge %g lds %d" % (radius, lds), src, dst, T, radius, tally, lds_points=lds, exact=True)
            assert d["inlier"][:n_on].all() and not d["inlier"][n_on:].any() and d["fitness"] == 0.5
            assert np.all(d["dist2"][:n_on] == radius * radius)
    eng.close()


def test_scan_size_edges(gpu_required):
    eng = _engine()
    tally = [0, 0]
    for n1 in S.SIZES_N1:
        for n2 in S.SIZES_N2:
            src, dst, init = S.size_pair(n1, n2, seed=1000 + n1 + n2)
            e, d = _scan(eng, "n1 %d n2 %d" % (n1, n2), src, dst, init, 0.1, tally)
            if n2 < 4:
                assert np.all(d["lanes"][:, n2:] == NONE)                     # empty slices
            if n2 > 8 and n2 < 4270:   # a small LDS stage: most of the cloud in the tail
                _scan(eng, "n1 %d n2 %d lds 7" % (n1, n2), src, dst, init, 0.1, tally, lds_points=7)
    assert tally[0] <= S.POINT_CAP * tally[1], tally
    # empty clouds: nothing chosen, nothing counted
    src, dst, init = S.size_pair(5, 9, seed=1)
    d = eng.debug_icp_scan(src, dst[:0], init)
    assert np.all(d["index"] == -1) and not d["inlier"].any() and d["fitness"] == 0.0 and d["rmse"] == 0.0
    d = eng.debug_icp_scan(src[:0], dst, init)
    assert d["index"].size == 0 and d["fitness"] == 0.0
    with pytest.raises(RuntimeError):
        eng.debug_icp_scan(src, dst, init, lds_points=S.LDS_BUDGET + 1)
    with pytest.raises(RuntimeError):
        eng.debug_icp_scan(src, dst, init, radius=0.0)
    eng.close()


@pytest.mark.parametrize("offset", S.OFFSETS)
def test_whole_runs_far_frames(gpu_required, offset):
    """The full iteration far from the origin (tests/test_icp_gpu.py::test_icp_exact_ties_and_far_frames compares one estimate there): host entry and
    rows entry, both estimate kinds, radius 0.1 and 0.02."""
    eng = _engine()
    pairs = [S.dense_pair(shape, n2, offset, True, S.WHOLE_SEED) for shape, n2 in S.WHOLE_RUN]
    src, dst, inits = [p[0] for p in pairs], [p[1] for p in pairs], [p[3] for p in pairs]
    off = np.zeros((len(src) + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(s) for s in src]); off[1:, 1] = np.cumsum([len(t) for t in dst])
    eng.upload_dataset(np.concatenate(src), np.concatenate(dst), off, np.zeros((len(src), 12), np.float32))
    scale = max(1.0, S.offset_norm(offset))
    skipped = 0
    for constrained in (True, False):
        for radius in (0.1, 0.02):
            res = eng.icp_refine(src, dst, inits, radius=radius, its=30, constrained=constrained)
            rows = eng.icp_refine_rows([2, 0, 1], [inits[2], inits[0], inits[1]], radius=radius, its=30, constrained=constrained)
            for k, r in enumerate((2, 0, 1)):
                assert np.array_equal(rows["transforms"][k], res["transforms"][r]) and rows["iterations"][k] == res["iterations"][r]
                assert rows["fitness"][k] == res["fitness"][r] and rows["rmse"][k] == res["rmse"][r]
            for k in range(len(src)):
                T, fit, rmse, it, und, _ = S.icp_with_margins(src[k], dst[k], inits[k], radius, 30, constrained)
                err = np.abs(res["transforms"][k] - T).max()
                print("offset %s %-5s constrained %d radius %.2f: %d iterations (device %d), %d undecided, transform error %.3g (bar %.3g), rmse error %.3g"
                      % (offset, S.WHOLE_RUN[k][0], constrained, radius, it, res["iterations"][k], und, err, 1e-9 * scale, abs(res["rmse"][k] - rmse)))
                if und:
                    skipped += 1
                    continue
                np.testing.assert_allclose(res["transforms"][k], T, rtol=0, atol=1e-9 * scale)
                assert res["fitness"][k] == fit and res["iterations"][k] == it and abs(res["rmse"][k] - rmse) < (1e-12 if offset == 0.0 else 1e-9)
    assert skipped <= 1
    eng.close()


def test_batch_geometry(gpu_required):
    """300 heterogeneous pairs in one call (more workgroups than CUs; empties in the middle; one pair with a tail) equal, bit for bit, the same pairs
    one at a time and in shuffled order, and match the restatement; lds_points (set by a call's largest target) does not change a pair's bits."""
    eng = _engine()
    srcs, dsts, inits = S.batch_pairs()
    n = len(srcs)
    key = lambda r, k: (r["transforms"][k].tobytes(), r["fitness"][k], r["rmse"][k], int(r["iterations"][k]))
    perm = np.random.default_rng(5).permutation(n)
    for constrained in (True, False):
        res = eng.icp_refine(srcs, dsts, inits, radius=0.1, its=3, constrained=constrained)
        shuf = eng.icp_refine([srcs[i] for i in perm], [dsts[i] for i in perm], [inits[i] for i in perm], radius=0.1, its=3, constrained=constrained)
        for k, i in enumerate(perm):
            assert key(shuf, k) == key(res, i), (constrained, i)
        small = [i for i in range(n) if len(dsts[i]) <= 700]                 # this call stages 700 targets, the full one 4266
        sub = eng.icp_refine([srcs[i] for i in small], [dsts[i] for i in small], [inits[i] for i in small], radius=0.1, its=3, constrained=constrained)
        for k, i in enumerate(small):
            assert key(sub, k) == key(res, i), (constrained, i)
        for i in range(n):
            one = eng.icp_refine([srcs[i]], [dsts[i]], [inits[i]], radius=0.1, its=3, constrained=constrained)
            assert key(one, 0) == key(res, i), (constrained, i)
        rank1 = 0
        for i in range(n):
            info = {}
            T, fit, rmse, it, und, _ = S.icp_with_margins(srcs[i], dsts[i], inits[i], 0.1, 3, constrained, info=info)
            assert und == 0
            if not constrained and info["rank2"] < 1e-9:
                # collinear correspondences (two points; every source point on one of two targets): a cross-covariance of rank 1 leaves the turn about
                # their line free (LAPACK's choice is as good as any), so a proper rotation is all that can be asked.  Rank 0 -- one correspondence, or
                # all on one target -- IS compared: both sides keep the rotation.  (Measured on the restatement: ratios are < 1e-15 or > 1e-3.)
                rank1 += 1
                R = res["transforms"][i][:3, :3]
                assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1) < 1e-12 and np.isfinite(res["transforms"][i]).all()
                # what IS determined: the device's own last evaluation (fitness, rmse) is the restatement's evaluation AT the device's transform, and
                # at that transform the correspondences' centroids coincide and their lines are aligned whenever an estimate was the last thing done
                ev = S.evaluate_with_margins(srcs[i], dsts[i], res["transforms"][i], 0.1)
                if not ev["undecided"].any():
                    assert res["fitness"][i] == ev["fitness"] and abs(res["rmse"][i] - ev["rmse"]) < 1e-12, i
                # one estimate from the restatement's correspondences: A = sum q' p'^T = sigma u v^T (rank 1), and the optimum maps v onto u
                e0 = S.evaluate_with_margins(srcs[i], dsts[i], inits[i], 0.1)
                if e0["inlier"].sum() >= 2 and not e0["undecided"].any():
                    one = eng.icp_refine([srcs[i]], [dsts[i]], [inits[i]], radius=0.1, its=1, constrained=False)
                    U = one["transforms"][0] @ np.linalg.inv(inits[i])
                    pp, qq = e0["p"][e0["inlier"]], dsts[i][e0["index"][e0["inlier"]]].astype(np.float64)
                    np.testing.assert_allclose((pp @ U[:3, :3].T + U[:3, 3]).mean(0), qq.mean(0), rtol=0, atol=1e-9)
                    Us, sv, Vt = np.linalg.svd((qq - qq.mean(0)).T @ (pp - pp.mean(0)))
                    if sv[0] > 0 and sv[1] < 1e-9 * sv[0]:
                        assert np.abs(U[:3, :3] @ Vt[0] - Us[:, 0]).max() < 1e-9, (i, U[:3, :3] @ Vt[0], Us[:, 0])
                continue
            np.testing.assert_allclose(res["transforms"][i], T, rtol=0, atol=1e-9, err_msg="pair %d" % i)
            assert res["fitness"][i] == fit and res["iterations"][i] == it and abs(res["rmse"][i] - rmse) < 1e-12, (i, len(srcs[i]), len(dsts[i]))
        print("batch, constrained %d: %d pairs compared with the restatement, %d with collinear correspondences held to properness" % (constrained, n - rank1, rank1))
        assert rank1 == (0 if constrained else S.BATCH_COLLINEAR)
    eng.close()


def test_estimate_branches(gpu_required):
    eng = _engine()
    for kind in ("mirror", "planar", "planar_noise"):
        src, dst, init = S.estimate_pair(kind, seed=5)
        e = S.evaluate_with_margins(src, dst, init, 0.1)
        want = F.estimate_full(e["p"], dst.astype(np.float64)) @ init
        res = eng.icp_refine([src], [dst], [init], radius=0.1, its=1, constrained=False)
        err = np.abs(res["transforms"][0] - want).max()
        print("%s: transform error %.3g, det R %.15f" % (kind, err, np.linalg.det(res["transforms"][0][:3, :3])))
        np.testing.assert_allclose(res["transforms"][0], want, rtol=0, atol=1e-9)
        T, fit, rmse, it = F.icp_p2point(src, dst, init, 0.1, 1)
        assert np.array_equal(T, want) and res["iterations"][0] == it == 1 and res["fitness"][0] == fit and abs(res["rmse"][0] - rmse) < 1e-12
    eng.close()


def test_estimate_keeps_rotation_when_none_is_determined(gpu_required):
    """Every source point on ONE target far from the pivot (the first target point): the cross-covariance is zero up to the rounding of its one-pass sums,
    no rotation is determined, and both estimates keep the rotation like the restatements (atan2(0, 0); the SVD of a zero matrix) instead of reading an
    angle out of the residue.  And the guard is not a floor on real signal: a covariance a million times smaller than the clouds' extent squared
    (two targets 1e-3 apart, 100 m from the pivot) still turns."""
    eng = _engine()
    rng = np.random.default_rng(9)
    for offset in (0.0, 100.0):
        far = np.array([[offset + 3.0, offset - 2.0, 1.0]])
        dst = np.concatenate([[[0.5, 0.25, 0.125]], far, far + [0.001, 0.0, 0.0], far + [0.0, 0.001, 0.0005]]).astype(np.float32)
        one = (far + rng.normal(0, 1e-5, (40, 3))).astype(np.float32)                       # all nearest to target 1
        two = (dst[1:4][rng.integers(3, size=40)].astype(np.float64) + rng.normal(0, 1e-5, (40, 3))).astype(np.float32)
        init = S.rigid_about(far[0], [0.0, 0.0, 0.02], [1e-5, -1e-5, 0.0])
        for constrained in (True, False):
            # (the 1 mm structure is summed about a pivot next to it -- the first target point -- as the kernel's one-pass sums are built for)
            for src, tgt, name in ((one, dst, "one target"), (two, dst[[1, 2, 3, 0]], "three targets 1 mm apart")):
                res = eng.icp_refine([src], [tgt], [init], radius=0.1, its=1, constrained=constrained)
                T, fit, rmse, it = F.icp_p2point(src, tgt, init, 0.1, 1, with_constraint=constrained)
                err = np.abs(res["transforms"][0] - T).max()
                print("offset %s %s constrained %d: transform error %.3g" % (offset, name, constrained, err))
                np.testing.assert_allclose(res["transforms"][0], T, rtol=0, atol=1e-9 * max(1.0, offset))
                assert res["fitness"][0] == fit and res["iterations"][0] == it
                if name == "one target":
                    assert np.array_equal(res["transforms"][0][:3, :3], init[:3, :3])       # the rotation is kept, bit for bit
    eng.close()
