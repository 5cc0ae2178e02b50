"""CPU: the inputs of tests/test_icp_scan_gpu.py on their own (tests/icp_scan_ref.py) -- the restatement with margins equals oracle/icp_ref.py's, the
inputs are as adversarial as claimed by measures that know nothing of the kernel (a float32 NumPy argmin against the fp64 one; gaps against need32),
every planted category is present in the stated number, and the caps of the GPU tests hide nothing: on the committed seeds the restatement alone
finds at most a tenth of POINT_CAP of the source points undecided and NO undecided pair in the whole runs.  Plus the read-back's header / ctypes
agreement."""
import os
import re

import numpy as np
import pytest

from oracle import icp_ref as I
from tests import icp_full_ref as F
from tests import icp_scan_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_back_declared_and_bound():
    from alignnet3d import _capi
    import alignnet3d
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alignnet_hip.h")).read(), flags=re.S)
    m = re.search(r"\balignnet_debug_icp_scan\s*\(([^)]*)\)", text)
    assert m and len(m.group(1).split(",")) == 16 == len(_capi.SYMBOLS["alignnet_debug_icp_scan"][1])
    assert int(re.search(r"#define\s+ALIGNNET_ABI_VERSION\s+(\d+)", text).group(1)) == _capi.ABI_VERSION == 1
    assert hasattr(alignnet3d.load_library(), "alignnet_debug_icp_scan") and callable(alignnet3d.Engine.debug_icp_scan)
    assert (150 * 1024) // 36 == S.LDS_BUDGET   # (tests/test_icp_scan_gpu.py checks the read-back's lds_points against it)


def test_restatement_with_margins_is_the_oracles():
    rng = np.random.default_rng(0)
    dst = rng.uniform(-1, 1, (700, 3)).astype(np.float32)
    dst[5] = dst[300]                                                       # a duplicate: an exact tie, the lower index wins, not undecided
    src = (dst[rng.permutation(700)[:400]] + rng.normal(0, 0.01, (400, 3))).astype(np.float32)
    src[0] = dst[300]
    T = S.rigid_about([0.1, 0.2, 0.3], [0.01, -0.02, 0.03], [0.004, 0.0, -0.003])
    e = S.evaluate_with_margins(src, dst, T, 0.1, rows=5000)               # (chunked: 7 source points at a time)
    p, q, fit, rmse = I._evaluate(src.astype(np.float64), dst.astype(np.float64), T, 0.1)
    assert np.array_equal(e["p"][e["inlier"]], p) and np.array_equal(dst[e["index"][e["inlier"]]].astype(np.float64), q)
    assert e["fitness"] == fit and e["rmse"] == rmse
    assert np.all(e["second"] > e["best"]) and np.all(e["gap"] > 0) and not e["undecided"].any()
    e1 = S.evaluate_with_margins(src[:1], dst, np.eye(4), 0.1)
    assert e1["index"][0] == 5 and e1["best"][0] == 0.0 and not e1["undecided"][0]
    for constrained in (True, False):
        a = S.icp_with_margins(src, dst, T, 0.1, 6, constrained)
        b = F.icp_p2point(src, dst, T, 0.1, 6, with_constraint=constrained)
        assert np.array_equal(a[0], b[0]) and a[1:4] == b[1:4] and a[4] == 0
    # the bounds: monotone, and of the size the derivation gives
    assert np.isclose(S.b64(4096.0, 1e-4), 2.0 ** -53 * (16 * np.sqrt(3) * 4096 * 1e-2 + 1e-3) + (8 * np.sqrt(3) * 2.0 ** -53 * 4096) ** 2)
    assert np.isclose(S.need32(4096.0, 1e-4), 2.0 ** -24 * (2 * np.sqrt(3) * 4096 * 1e-2 + 5e-4))
    assert S.need32(50.0, 0.0025) / 8 > 1e3 * S.UNDECIDED * S.b64(50.0, 0.0025)     # the planted band is wide: three decades and more
    # an undecided point is found when there is one: two targets whose distances differ in the last bits
    near = np.array([[0.0, 0.0, 0.0], [2.0 ** -5, 0.0, 0.0]], np.float32)
    mid = np.array([[2.0 ** -6, 0.0, 0.0]], np.float32) + 4096
    e2 = S.evaluate_with_margins(mid, near + 4096, S.rigid_about([4096] * 3, [0.0, 0.0, 0.0], [1e-9, 0, 0]), 0.1)
    assert e2["undecided"][0] and 0 < e2["gap"][0] < 1e-10 and e2["index"][0] == 1
    e2 = S.evaluate_with_margins(mid, near + 4096, S.rigid_about([4096] * 3, [0.0, 0.0, 0.0], [1e-5, 0, 0]), 0.1)
    assert not e2["undecided"][0]


def test_dense_inputs_are_adversarial_and_decided():
    und = tot = 0
    for shape, n2, off, gen in S.dense_cases():
        src, dst, T, _ = S.dense_pair(shape, n2, off, gen, S.DENSE_SEED)
        e = S.evaluate_with_margins(src, dst, T, 0.02)
        wrong = float(((S.fp32_argmin(src, dst, T) != e["index"]) & (e["gap"] > 0)).mean())
        unresolved = float((e["gap"] < S.need32(e["P32"], e["second"])).mean())
        print("%-5s n2 %d offset %s general %d: %d points, %d undecided, float32 argmin wrong %.2f %%, gap < need32 %.1f %%, fitness %.3f"
              % (shape, n2, off, gen, len(src), e["undecided"].sum(), 100 * wrong, 100 * unresolved, e["fitness"]))
        und += int(e["undecided"].sum()); tot += len(src)
        assert len(src) == int(0.7 * n2) and e["fitness"] == 1.0
        if gen and off == 4096.0 and shape in ("cube", "sheet"):
            assert wrong >= 0.01 and unresolved >= 0.15, (shape, n2, wrong, unresolved)
        if gen and off == 4096.0 and shape == "lines":     # 2 - 5 mm along a line against 0.24 mm of float32 rounding: fewer, but there
            assert wrong >= 0.0025 and unresolved >= 0.015, (shape, n2, wrong, unresolved)
        if gen and S.offset_norm(off) >= 512.0 and shape != "lines":
            assert wrong >= 0.002, (shape, n2, off, wrong)
    assert und <= S.POINT_CAP / 10 * tot, (und, tot)


@pytest.mark.parametrize("offset", [0.0, 50.0])
def test_planted_near_ties_are_what_they_claim(offset):
    src, dst, T, plan = S.planted_pair(offset, seed=3)
    e = S.evaluate_with_margins(src, dst, T, S.PLANT_RADIUS)
    assert not e["undecided"].any()
    assert np.array_equal(e["index"], plan["near"]) and np.allclose(e["gap"], plan["gap"], rtol=1e-9, atol=0)
    far_d = ((e["p"] - dst[plan["far"]].astype(np.float64)) ** 2).sum(1)
    assert np.allclose(far_d, e["second"], rtol=1e-12, atol=0)               # the second smallest distance is the planted partner's
    zero = plan["rclass"] == 0
    hi = S.need32(e["P32"], e["second"])
    assert np.all(e["gap"] >= S.UNDECIDED * S.b64(e["P64"], e["second"]))
    assert np.all(e["gap"][~zero] <= hi[~zero] / 8) and np.all(e["gap"][zero] <= hi[zero])
    assert np.all(e["p"][zero].astype(np.float32) == dst[plan["near"][zero]])      # the float32 scan sees distance 0 there
    lg = np.log10(e["gap"][~zero])
    assert np.histogram(lg, bins=6)[0].min() >= 10 and lg.max() - lg.min() > 3.0, np.histogram(lg, bins=6)   # spread over the band's decades
    names = np.array(S.PLANT_R)[plan["rclass"]]
    assert e["inlier"][names != "outside"].all() and not e["inlier"][names == "outside"].any()
    assert np.all(np.abs(e["best"][names == "inside"] - S.PLANT_RADIUS ** 2) < S.need32(e["P32"], e["best"])[names == "inside"])
    assert np.all(np.abs(e["best"][names == "outside"] - S.PLANT_RADIUS ** 2) < S.need32(e["P32"], e["best"])[names == "outside"])
    near, far, L = plan["near"], plan["far"], S.PLANT_LDS
    where = {"same_slice": (near % 4 == far % 4) & (near < L) & (far < L), "cross_slice": (near % 4 != far % 4) & (near < L) & (far < L),
             "lds_tail": (np.minimum(near, far) < L) & (np.maximum(near, far) >= L), "both_tail": (near >= L) & (far >= L)}
    for c, name in enumerate(S.PLANT_CATEGORIES):
        for order in (0, 1):
            sel = (plan["category"] == c) & (plan["order"] == order)
            assert sel.sum() >= 32 and where[name][sel].all() and np.all((near[sel] < far[sel]) == (order == 0)), (name, order)
            assert len(set(plan["rclass"][sel])) == len(S.PLANT_R)


@pytest.mark.parametrize("offset", [0.0, 50.0])
def test_planted_three_and_four_way_near_ties_are_what_they_claim(offset):
    src, dst, T, plan = S.planted_multi(offset, seed=4)
    e = S.evaluate_with_margins(src, dst, T, S.PLANT_RADIUS)
    assert not e["undecided"].any() and np.array_equal(e["index"], plan["idx"][:, 0]) and e["inlier"].all()
    L = S.PLANT_LDS
    for k in range(len(src)):
        m = int(plan["m"][k])
        j = plan["idx"][k, :m]
        d = ((e["p"][k] - dst[j].astype(np.float64)) ** 2).sum(1)
        assert (plan["idx"][k, m:] == -1).all() and np.all(np.diff(d) >= S.UNDECIDED * S.b64(e["P64"][k], d[-1]))       # fp64 orders them all
        assert d[-1] - d[0] <= S.need32(e["P32"][k], d[-1]) / 8 and np.isclose(d[-1] - d[0], plan["span"][k], rtol=1e-9)   # fp32 orders none
        others = np.delete(((e["p"][k] - dst.astype(np.float64)) ** 2).sum(1), j)
        assert others.min() > 0.01                                            # the fillers are nowhere near
        lay = S.MULTI_LAYOUTS[plan["layout"][k]]
        if lay == "same_slice":
            assert len(set(j % 4)) == 1 and (j < L).all()
        elif lay == "spread":
            assert len(set(j % 4)) == m and (j < L).all()
        else:
            assert (j < L).sum() == 2 and len(set(j[j < L] % 4)) == 2 and (j >= L).sum() == m - 2
    for m in (3, 4):
        for lay in range(len(S.MULTI_LAYOUTS)):
            sel = (plan["m"] == m) & (plan["layout"] == lay)
            first = plan["idx"][sel, 0]
            assert sel.sum() >= 32 and (first == plan["idx"][sel, :m].min(1)).sum() >= 4 and (first == plan["idx"][sel, :m].max(1)).sum() >= 4, (m, lay)
    assert (plan["idx"][:, 0] >= L).sum() >= 16


def test_radius_edge_is_exact():
    for radius in (2.0 ** -4, 2.0 ** -3):
        src, dst, T, n_on = S.radius_edge_pair(radius)
        e = S.evaluate_with_margins(src, dst, T, radius, exact=True)
        # in integers: coordinates are multiples of 2^-27 below 2 (a float32 ulp under 1 is >= 2^-24 ... 2^-27 in [1/16, 1])
        si, di = np.round(src.astype(np.float64) * 2.0 ** 27).astype(np.int64), np.round(dst.astype(np.float64) * 2.0 ** 27).astype(np.int64)
        assert np.array_equal(si / 2.0 ** 27, src.astype(np.float64)) and np.array_equal(di / 2.0 ** 27, dst.astype(np.float64))
        d2 = ((si[:, None, :] - di[None, :, :]) ** 2).sum(-1)               # < 2^58: exact
        assert np.array_equal(d2.argmin(1), e["index"]) and np.array_equal(d2.min(1) / 2.0 ** 54, e["best"])
        assert np.all(d2.min(1)[:n_on] == int(radius * 2 ** 27) ** 2) and np.all(d2.min(1)[n_on:] > int(radius * 2 ** 27) ** 2)
        assert e["inlier"][:n_on].all() and not e["inlier"][n_on:].any() and n_on == 24
        assert np.all((d2 == d2.min(1)[:, None]).sum(1) == 1)              # their only candidate


def test_size_edges_batch_and_usefulness_inputs_are_decided():
    und = tot = 0
    for n1 in S.SIZES_N1:
        for n2 in S.SIZES_N2:
            src, dst, init = S.size_pair(n1, n2, seed=1000 + n1 + n2)
            e = S.evaluate_with_margins(src, dst, init, 0.1)
            und += int(e["undecided"].sum()); tot += n1
            if n2 == 8533:   # exact ties across the LDS / tail border are there, and sources whose nearest target lies only in the tail
                assert (e["index"][: min(n1, 40)] < S.LDS_BUDGET).all() and (np.isfinite(e["second"][: min(n1, 40)])).all()
                dup = (dst[e["index"]] == dst[:, None][S.LDS_BUDGET:]).all(-1).any(0)
                assert n1 < 255 or (dup.sum() >= 40 and (e["index"] >= S.LDS_BUDGET).sum() >= 40), (n1, dup.sum())
    assert und <= S.POINT_CAP / 10 * tot, (und, tot)
    srcs, dsts, inits = S.batch_pairs()
    assert len(srcs) == 300 and sum(len(d) > S.LDS_BUDGET for d in dsts) == 1 and sum(len(s) == 0 for s in srcs) == 2 and sum(len(d) == 0 for d in dsts) == 2
    for constrained in (True, False):
        collinear = 0
        for k in range(300):
            info = {}
            assert S.icp_with_margins(srcs[k], dsts[k], inits[k], 0.1, 3, constrained, info=info)[4] == 0
            assert info["rank2"] < 1e-14 or info["rank2"] > 1e-3, (k, info)       # collinear correspondences or clearly not: nothing in between
            collinear += info["rank2"] < 1e-9
        assert collinear == S.BATCH_COLLINEAR       # (every 2-point source on two targets, every source on a 2-point target, 3 points on 2 targets)
    # the usefulness check's input: nearly every source point of the existing tests' clouds has its second target FAR beyond what fp32 blurs
    from tests.test_icp_gpu import _pairs
    src, dst, inits, _ = _pairs(7, seed=2)
    clear = n = 0
    for k in range(7):
        e = S.evaluate_with_margins(src[k], dst[k], inits[k], 0.1)
        clear += int((e["gap"] > 1000 * S.need32(e["P32"], e["second"])).sum()); n += len(src[k])
        assert not e["undecided"].any()
    print("usefulness input: %d of %d source points have gap > 1000 need32" % (clear, n))
    assert n == 2421 and clear >= 0.99 * n


@pytest.mark.parametrize("offset", S.OFFSETS)
def test_whole_run_inputs_have_no_undecided_pair(offset):
    for shape, n2 in S.WHOLE_RUN:
        src, dst, _, init = S.dense_pair(shape, n2, offset, True, S.WHOLE_SEED)
        for constrained in (True, False):
            for radius in (0.1, 0.02):
                T, fit, rmse, k, und, evals = S.icp_with_margins(src, dst, init, radius, 30, constrained)
                print("offset %s %-5s constrained %d radius %.2f: %d iterations, %d undecided points in %d evaluations, fitness %.3f rmse %.2e"
                      % (offset, shape, constrained, radius, k, und, evals, fit, rmse))
                assert und == 0 and k >= 2 and fit > 0.9


def test_estimate_branch_inputs_take_their_branch():
    for kind in ("mirror", "planar", "planar_noise"):
        src, dst, init = S.estimate_pair(kind, seed=5)
        e = S.evaluate_with_margins(src, dst, init, 0.1)
        assert e["inlier"].all() and np.array_equal(e["index"], np.arange(len(src))) and not e["undecided"].any()
        p, q = e["p"], dst.astype(np.float64)
        Sg = (q - q.mean(0)).T @ (p - p.mean(0)) / len(p)
        U, sv, Vt = np.linalg.svd(Sg)
        print(kind, "singular values", sv, "det U det V", np.linalg.det(U) * np.linalg.det(Vt))
        assert sv[0] > 2 * sv[1] and sv[1] > 100 * sv[2]
        if kind == "mirror":
            assert np.linalg.det(Sg) < 0 and np.linalg.det(U) * np.linalg.det(Vt) < 0       # estimate_full takes D = diag(1, 1, -1)
            assert sv[2] > 1e-5
        if kind == "planar":
            assert np.all(p[:, 2] == 0.5) and np.all(q[:, 2] == 0.5) and sv[2] < 1e-20
        R = F.estimate_full(p, q)[:3, :3]
        assert abs(np.linalg.det(R) - 1) < 1e-12 and np.allclose(R @ R.T, np.eye(3), atol=1e-12)
