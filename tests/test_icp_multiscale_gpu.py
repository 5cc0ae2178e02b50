"""GPU: multi-scale ICP (Engine.icp_multiscale_refine*, csrc/alignnet_multiscale.hip) against tests/icp_multiscale_ref.py.
1. The pyramid through Engine.debug_voxel_pyramid (the shipped kernels with a record behind them): voxel indices and counts equal, fp64 means within
   1e-12 relative, the float32 cloud equal to float32(device mean) exactly.  The device and the restatement perform the same IEEE fp64 operations, so
   nothing is skipped; the inputs keep away from voxel faces (tests/test_icp_multiscale_cpu.py) except the lattice, which sits on them exactly.
2. A whole call equals, bit for bit, the composition a user could write: level clouds read back, Engine.icp_refine / icp_plane_refine /
   icp_generalized_refine level by level with the level before's output as init.
3. Every level against the restatement, fed the device's own level clouds and input transform: transforms within 1e-9 max(1, |offset|), rmse within
   1e-9, fitness and iterations equal; a level with an undecided entry is left out under the restatements' caps.
4. Edges and bad arguments.  5. The drop-in."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import alignnet3d
from alignnet3d import EngineError
from tests import icp_multiscale_ref as M
from tests import icp_plane_ref as P
from tests import icp_scan_ref as S
from tests.helpers import small_cfg
from tests.test_icp_plane_gpu import _make_dataset, _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
REFINE = {"point": "icp_refine", "plane": "icp_plane_refine", "generalized": "icp_generalized_refine"}
SEARCH = {"scan": 0, "grid": 1, "auto": 2}
# the kernel's internal borders (csrc/alignnet_multiscale.hip): 1,024 threads take one record each up to 1,024 points; the LDS sort pads to a power of
# two (2,048); clouds above kMsChunk = 8,192 records sort in chunks through HBM; 16,384 = two full chunks, one more point opens a third
BORDER_SIZES = (1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385)


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _car():
    return M.car_scan()


@functools.lru_cache(maxsize=None)
def _small(k):
    seed, dist = M.SMALL_PAIRS[k]
    return P.car_pair(dist, seed)


def _box(n, seed, lo=-3.0, hi=3.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def _check_pyramid(eng, name, pc, voxels):
    dev = eng.debug_voxel_pyramid(pc, voxels)
    ref = M.pyramid(pc, voxels)
    assert len(dev) == len(voxels)
    for v, d, r in zip(voxels, dev, ref):
        if not v > 0:
            assert np.array_equal(d["points"], np.asarray(pc, np.float32).reshape(-1, 3)) and d["voxels"] is None
            continue
        worst = float(np.max(np.abs(d["means"] - r["means"]) / np.maximum(np.abs(r["means"]), 1e-300))) if len(r["means"]) == len(d["means"]) and len(r["means"]) else 0.0
        print("%s at %g: %d points -> %d voxels (restatement %d), means differ by %.1e relative" % (name, v, len(pc), len(d["points"]), len(r["points"]), worst))
        assert np.array_equal(d["voxels"], r["voxels"]), (name, v)
        assert np.array_equal(d["counts"], r["counts"]), (name, v)
        np.testing.assert_allclose(d["means"], r["means"], rtol=M.MEAN_TOL, atol=0, err_msg="%s at %g" % (name, v))
        assert np.array_equal(d["points"], d["means"].astype(np.float32)), (name, v)
    return dev


# ---- 1. the pyramid ------------------------------------------------------------------------------------------------------------------------------
def test_pyramid_car_scan(eng):
    src, dst, _ = _car()
    for name, pc in (("car source", src), ("car target", dst)):
        for v in M.CAR_VOXELS:
            assert M.undecided_share(pc, v) <= M.FACE_CAP
        _check_pyramid(eng, name, pc, M.CAR_VOXELS + (0.0,))
    assert eng.get_option("icp_multiscale_ws_bytes") >= 4 * len(dst) * 24


def test_pyramid_exact_lattice(eng):
    """Every operation exact and seven in eight points ON a voxel face: the assignment is floor's closed lower face, nothing skipped."""
    pc = M.lattice()
    assert M.on_face_share(pc, 0.125) > 0.86
    dev = _check_pyramid(eng, "lattice", pc, (0.5, 0.25, 0.125))
    for d, r in zip(dev, M.pyramid(pc, (0.5, 0.25, 0.125))):
        assert np.array_equal(d["means"], r["means"])        # (sums of multiples of 2^-4 are exact; the division rounds once on both sides)


def test_pyramid_tiny_and_degenerate(eng):
    rng = np.random.default_rng(2)
    for v in (0.3, 0.05):
        levels = eng.debug_voxel_pyramid(np.zeros((0, 3), np.float32), [v, 0.0])
        assert len(levels[0]["points"]) == 0 and len(levels[0]["counts"]) == 0 and len(levels[1]["points"]) == 0
    one = np.array([[1.25, -2.5, 0.75]], np.float32)
    _check_pyramid(eng, "one point", one, (0.3, 0.05))
    _check_pyramid(eng, "two points apart", np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]], np.float32), (0.3, 0.05))
    _check_pyramid(eng, "two points together", np.array([[0.0, 0.0, 0.0], [0.01, 0.02, 0.03]], np.float32), (0.3,))
    blob = (one + rng.uniform(0, 0.001, (500, 3))).astype(np.float32)
    dev = _check_pyramid(eng, "all in one voxel", blob, (0.3,))
    assert len(dev[0]["points"]) == 1 and dev[0]["counts"][0] == 500
    alone = (rng.permutation(3000)[:, None] * np.array([[0.5, 0.0, 0.0]]) + rng.uniform(0.1, 0.2, (3000, 3))).astype(np.float32)
    dev = _check_pyramid(eng, "every point alone", alone, (0.3,))
    assert len(dev[0]["points"]) == 3000 and np.all(dev[0]["counts"] == 1)
    base = _box(700, 3)
    dup = np.concatenate([base, base[::2], base[::3], base])[rng.permutation(700 + 350 + 234 + 700)]
    dev = _check_pyramid(eng, "duplicated points", dup, (0.37, 0.11))
    assert dev[1]["counts"].sum() == len(dup)


@pytest.mark.parametrize("n", BORDER_SIZES)
def test_pyramid_border_sizes(eng, n):
    pc = _box(n, n)
    for v in (0.53, 0.11):
        assert M.undecided_share(pc, v) <= M.FACE_CAP
    _check_pyramid(eng, "box of %d" % n, pc, (0.53, 0.11))


def test_pyramid_70000_points(eng):
    pc = _box(70000, 9, -10.0, 10.0)
    assert M.undecided_share(pc, 0.8) <= M.FACE_CAP and M.undecided_share(pc, 0.23) <= M.FACE_CAP
    _check_pyramid(eng, "70,000 points", pc, (0.8, 0.23))


def test_pyramid_far_frame(eng):
    """At (4000, -3000, 50) m float32 coordinates are 2.4e-4 m apart: an fp32 floor, or a reciprocal in place of the division, bins them elsewhere."""
    pc = M.far_cloud()
    for v in M.FAR_VOXELS:
        assert M.undecided_share(pc, v) <= M.FACE_CAP
    _check_pyramid(eng, "far cloud", pc, M.FAR_VOXELS)


def test_pyramid_voxel_span_and_not_finite(eng):
    """One point 100,000 m away at 0.05: 2,000,000 voxels on an axis, inside the limit.  110,000 m are more than 2^21: refused, nothing truncated, and
    the next good call returns what it returned before.  A NaN or infinite coordinate is refused the same way."""
    body = _box(200, 4, 0.0, 1.0)
    good = np.concatenate([body, [[100000.0, 0.5, 0.5]]]).astype(np.float32)
    before = _check_pyramid(eng, "2,000,000 voxels wide", good, (0.05, 0.4))
    assert before[0]["voxels"][:, 0].max() >= 2000000
    src, dst, truth = _small(0)
    init = M.disturbed_init(src, truth, 1)
    sched = ([0.05, 0.0], [0.3, 0.1], [4, 4])                   # (110,000 m are 2,200,000 voxels of 0.05)
    ok = eng.icp_multiscale_refine([src], [dst], [init], *sched)
    wide = np.concatenate([body, [[110000.0, 0.5, 0.5]]]).astype(np.float32)
    nan = body.copy(); nan[17, 1] = np.nan
    inf = body.copy(); inf[3, 2] = -np.inf
    for bad in (wide, nan, inf):
        with pytest.raises(EngineError, match=r"2\^21 voxels"):
            eng.debug_voxel_pyramid(bad, (0.05,))
        for s, d in ((bad, dst), (src, bad)):
            with pytest.raises(EngineError, match=r"2\^21 voxels"):
                eng.icp_multiscale_refine([src, s], [dst, d], [init, init], *sched)
        eng.debug_voxel_pyramid(wide, (0.4,))       # the same cloud at a voxel size that spans it
        again = eng.debug_voxel_pyramid(good, (0.05, 0.4))
        for a, b in zip(before, again):
            assert all(np.array_equal(a[k], b[k]) for k in ("points", "means", "voxels", "counts"))
        res = eng.icp_multiscale_refine([src], [dst], [init], *sched)
        assert all(np.array_equal(ok[k], res[k]) for k in ok)


def test_pyramid_heterogeneous_batch(eng):
    """[large, 3 points, empty, car] in one call: every level cloud is bit for bit the cloud's alone -- shown by the evaluation (its = 0: fitness and
    rmse of the given transform on the level's clouds at its radius) of the batch against each pair alone, in both batch positions and as source
    and as target, and by the level sizes against the read-back."""
    src, dst, truth = _small(1)
    clouds = [_box(20000, 6), _box(3, 7), np.zeros((0, 3), np.float32), src]
    partner = [_box(20000, 6)[::3] + np.float32(0.01), _box(3, 7), src, dst]
    inits = [np.eye(4), np.eye(4), np.eye(4), truth]
    voxels = [0.31, 0.12]
    sizes = np.array([[len(l["points"]) for l in eng.debug_voxel_pyramid(c, voxels)] for c in clouds])
    psizes = np.array([[len(l["points"]) for l in eng.debug_voxel_pyramid(c, voxels)] for c in partner])
    for last in range(2):
        sched = (voxels[:last + 1], [0.4, 0.2][:last + 1], [0, 0][:last + 1])
        for order in ((0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1)):
            S_, D_, I_ = [clouds[i] for i in order], [partner[i] for i in order], [inits[i] for i in order]
            both = eng.icp_multiscale_refine(S_, D_, I_, *sched)
            swapped = eng.icp_multiscale_refine(D_, S_, I_, *sched)
            assert np.array_equal(both["level_sizes"][:, :, 0], sizes[list(order), :last + 1]) and np.array_equal(both["level_sizes"][:, :, 1], psizes[list(order), :last + 1])
            for k, i in enumerate(order):
                one = eng.icp_multiscale_refine([clouds[i]], [partner[i]], [inits[i]], *sched)
                two = eng.icp_multiscale_refine([partner[i]], [clouds[i]], [inits[i]], *sched)
                for key in both:
                    assert np.array_equal(both[key][k], one[key][0]), (order, i, key)
                    assert np.array_equal(swapped[key][k], two[key][0]), (order, i, key)
    assert both["fitness"][list(order).index(3)] > 0.5      # (the car pair at its truth: the comparison is not of zeros)


# ---- 2. chaining, exact --------------------------------------------------------------------------------------------------------------------------
def _compose(eng, srcs, dsts, inits, voxels, radii, its, estimate, normal_radius, constrained):
    """What a user could write today: level clouds from the read-back, the single-scale refine level by level."""
    L = len(voxels)
    ps, pd = [eng.debug_voxel_pyramid(s, voxels) for s in srcs], [eng.debug_voxel_pyramid(d, voxels) for d in dsts]
    T = np.array(inits, np.float64)
    iters = np.zeros((len(srcs), L), np.int32)
    sizes = np.zeros((len(srcs), L, 2), np.int32)
    nr = np.broadcast_to(np.asarray(normal_radius, np.float64).reshape(-1), (L,))
    r = None
    for l in range(L):
        S_, D_ = [p[l]["points"] for p in ps], [p[l]["points"] for p in pd]
        kw = dict(radius=radii[l], its=its[l], constrained=constrained)
        if estimate != "point":
            kw["normal_radius"] = float(nr[l])
        r = getattr(eng, REFINE[estimate])(S_, D_, T, **kw)
        T = r["transforms"]
        iters[:, l] = r["iterations"]
        sizes[:, l, 0], sizes[:, l, 1] = [len(x) for x in S_], [len(x) for x in D_]
    return dict(transforms=T, fitness=r["fitness"], rmse=r["rmse"], iterations=iters, level_sizes=sizes)


def _same(a, b, what):
    for k in ("transforms", "fitness", "rmse", "iterations", "level_sizes"):
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


SCHEDULES = (([0.0], [0.1], [5]), ([0.2], [0.3], [5]), ([0.2, 0.0], [0.3, 0.1], [4, 4]), ([0.0, 0.1], [0.3, 0.1], [3, 3]),
             ([0.4, 0.1, -1.0], [0.5, 0.2, 0.1], [4, 3, 3]), ([0.4, 0.2, 0.1], [0.5, 0.3, 0.15], [3, 3, 3]))


@pytest.fixture(scope="module")
def chain_pairs(eng):
    """Two small car pairs and the 13,289 / 11,710-point one (beyond the scan's LDS stage: "auto" sends its raw level to the grid), uploaded as rows."""
    pairs = [_small(0), _small(1), _car()]
    srcs, dsts = [p[0] for p in pairs], [p[1] for p in pairs]
    inits = [M.disturbed_init(p[0], p[2], 10 + k) for k, p in enumerate(pairs)]
    off = np.zeros((len(pairs) + 1, 2), np.int64)
    off[1:, 0], off[1:, 1] = np.cumsum([len(s) for s in srcs]), np.cumsum([len(d) for d in dsts])
    eng.upload_dataset(np.concatenate(srcs), np.concatenate(dsts), off, np.zeros((len(pairs), 12), np.float32))
    return srcs, dsts, inits


@pytest.mark.parametrize("constrained", (True, False))
@pytest.mark.parametrize("estimate", ("point", "plane", "generalized"))
def test_call_equals_the_composition_bit_for_bit(eng, chain_pairs, estimate, constrained):
    srcs, dsts, inits = chain_pairs
    rows = [2, 0, 1, 0]                                           # (a row twice, the rows out of order)
    try:
        for search in (("scan", "grid", "auto") if estimate == "point" else ("scan",)):      # (plane and generalized always take the grid)
            eng.set_option("icp_search", SEARCH[search])
            for sched in SCHEDULES:
                nr = 0.3 if len(sched[0]) != 3 else [0.6, 0.4, 0.3]
                what = (estimate, constrained, search, sched)
                want = _compose(eng, srcs, dsts, inits, *sched, estimate, nr, constrained)
                host = eng.icp_multiscale_refine(srcs, dsts, inits, *sched, estimate=estimate, normal_radius=nr, constrained=constrained)
                _same(host, want, what)
                by_rows = eng.icp_multiscale_refine_rows(rows, [inits[i] for i in rows], *sched, estimate=estimate, normal_radius=nr, constrained=constrained)
                _same(by_rows, {k: v[rows] for k, v in want.items()}, what + ("rows",))
            assert host["iterations"].sum() > 0 and not np.array_equal(host["transforms"], np.array(inits))
    finally:
        eng.set_option("icp_search", 0)


# ---- 3. against the restatement ------------------------------------------------------------------------------------------------------------------
def _check_levels(eng, name, src, dst, init, voxels, radii, its, estimate, constrained, offset, tally):
    """Every level of one pair: the device's transform before the level (the call cut after the level before), its level clouds, the restatement."""
    ps, pd = eng.debug_voxel_pyramid(src, voxels), eng.debug_voxel_pyramid(dst, voxels)
    T_in = np.array(init, np.float64)
    cap = S.POINT_CAP if estimate == "point" else P.SKIP_CAP
    for l in range(len(voxels)):
        dev = eng.icp_multiscale_refine([src], [dst], [init], voxels[:l + 1], radii[:l + 1], its[:l + 1], estimate=estimate, normal_radius=0.3, constrained=constrained)
        T, fit, rmse, k, und, ent = M.run_level(ps[l]["points"], pd[l]["points"], T_in, radii[l], its[l], estimate, 0.3, constrained)
        tally[0] += und; tally[1] += ent
        dT = np.abs(dev["transforms"][0] - T).max()
        print("%s %s level %d (voxel %g, %d x %d points): iterations %d / %d, fitness %.4f / %.4f, rmse differs by %.1e, transform by %.1e, undecided %d of %d"
              % (name, estimate, l, voxels[l], len(ps[l]["points"]), len(pd[l]["points"]), dev["iterations"][0, l], k, dev["fitness"][0], fit,
                 abs(dev["rmse"][0] - rmse), dT, und, ent))
        assert dev["level_sizes"][0, l].tolist() == [len(ps[l]["points"]), len(pd[l]["points"])]
        if und == 0:
            tally[2] += 1
            assert dev["iterations"][0, l] == k and dev["fitness"][0] == fit, (name, l)
            assert abs(dev["rmse"][0] - rmse) <= 1e-9, (name, l)
            assert dT <= 1e-9 * max(1.0, offset), (name, l)
        else:
            assert und <= cap * ent, (name, l, und, ent)
        tally[3] += 1
        T_in = dev["transforms"][0]


@pytest.mark.parametrize("estimate", ("point", "plane", "generalized"))
def test_levels_against_the_restatement(eng, estimate):
    tally = [0, 0, 0, 0]
    cap = S.POINT_CAP if estimate == "point" else P.SKIP_CAP
    for k in range(len(M.SMALL_PAIRS)):
        src, dst, truth = _small(k)
        init = M.disturbed_init(src, truth, 20 + k)
        constrained = k != 1
        _check_levels(eng, "small %d" % k, src, dst, init, [0.2, 0.1, 0.0], [0.4, 0.2, 0.1], [8, 6, 5], estimate, constrained, 1.0, tally)
    src, dst, truth = M.far_pair()
    init = M.disturbed_init(src, truth, 30)
    _check_levels(eng, "4 km out", src, dst, init, [M.FAR_VOXELS[1], M.FAR_VOXELS[2], 0.0], [0.4, 0.2, 0.1], [8, 6, 5], estimate, True, float(np.linalg.norm(M.FAR)), tally)
    print("%s: %d of %d entries undecided, %d of %d levels compared" % (estimate, tally[0], tally[1], tally[2], tally[3]))
    assert tally[0] <= cap * tally[1] and 2 * tally[2] >= tally[3]


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------------------------
def test_edges(eng):
    src, dst, truth = _small(1)
    init = M.disturbed_init(src, truth, 41)
    empty = np.zeros((0, 3), np.float32)
    for estimate in ("point", "plane", "generalized"):
        # a level that only evaluates, in the middle and at the end
        for sched in (([0.2, 0.1, 0.0], [0.4, 0.2, 0.1], [4, 0, 3]), ([0.2, 0.0], [0.4, 0.1], [4, 0]), ([0.0], [0.1], [0])):
            got = eng.icp_multiscale_refine([src], [dst], [init], *sched, estimate=estimate)
            _same(got, _compose(eng, [src], [dst], [init], *sched, estimate, 0.3, True), (estimate, sched))
            assert all(got["iterations"][0, l] == 0 for l, n in enumerate(sched[2]) if n == 0)
        # an empty source, an empty target: the init comes back, nothing iterates
        for s, d in ((empty, dst), (src, empty), (empty, empty)):
            got = eng.icp_multiscale_refine([s, src], [d, dst], [init, init], [0.2, 0.0], [0.4, 0.1], [4, 4], estimate=estimate)
            assert np.array_equal(got["transforms"][0], init) and got["iterations"][0].tolist() == [0, 0] and got["fitness"][0] == 0.0 and got["rmse"][0] == 0.0
            assert got["level_sizes"][0, :, 0].tolist() == ([0, 0] if len(s) == 0 else [got["level_sizes"][1, 0, 0], len(src)])
            _same({k: v[1:] for k, v in got.items()}, eng.icp_multiscale_refine([src], [dst], [init], [0.2, 0.0], [0.4, 0.1], [4, 4], estimate=estimate), estimate)
        # a voxel that swallows the cloud: one point per side
        sched = ([100.0, 0.0], [5.0, 0.1], [3, 3])
        got = eng.icp_multiscale_refine([src], [dst], [init], *sched, estimate=estimate)
        assert got["level_sizes"][0, 0].tolist() == [1, 1]
        _same(got, _compose(eng, [src], [dst], [init], *sched, estimate, 0.3, True), (estimate, "one point"))


def test_300_pairs_in_one_call_equal_one_at_a_time(eng):
    srcs, dsts, inits = S.batch_pairs(300)
    sched = ([0.15, 0.0], [0.3, 0.1], [3, 3])
    for constrained in (True, False):
        got = eng.icp_multiscale_refine(srcs, dsts, inits, *sched, constrained=constrained)
        for b in range(300):
            one = eng.icp_multiscale_refine([srcs[b]], [dsts[b]], [inits[b]], *sched, constrained=constrained)
            for k in got:
                assert np.array_equal(got[k][b], one[k][0]), (b, k, constrained)
    assert got["iterations"].sum() > 300


def test_bad_arguments_launch_nothing(eng):
    src, dst, truth = _small(0)
    init = M.disturbed_init(src, truth, 51)
    good = ([0.2, 0.0], [0.4, 0.1], [4, 4])
    before = eng.icp_multiscale_refine([src], [dst], [init], *good)
    used = eng.get_option("icp_multiscale_ws_bytes")
    bad = (([], [], []), ([0.1] * 9, [0.1] * 9, [1] * 9), ([0.2, 0.0], [0.4, 0.0], [4, 4]), ([0.2, 0.0], [0.4, -0.1], [4, 4]),
           ([0.2, 0.0], [0.4, float("nan")], [4, 4]), ([0.2, 0.0], [0.4, 0.1], [4, -1]), ([float("nan"), 0.0], [0.4, 0.1], [4, 4]),
           ([float("inf"), 0.0], [0.4, 0.1], [4, 4]))
    for sched in bad:
        with pytest.raises(EngineError, match="L must be|radii|its|voxel_sizes"):
            eng.icp_multiscale_refine([src], [dst], [init], *sched)
    with pytest.raises(ValueError):
        eng.icp_multiscale_refine([src], [dst], [init], [0.2], [0.4, 0.1], [4])
    with pytest.raises(ValueError):
        eng.icp_multiscale_refine([src], [dst], [init], *good, estimate="gicp")
    for estimate in ("plane", "generalized"):
        with pytest.raises(EngineError, match="normal_radii"):
            eng.icp_multiscale_refine([src], [dst], [init], *good, estimate=estimate, normal_radius=[0.3, 0.0])
    # null lists, an unknown estimate and unknown flags through the C entry point
    import ctypes as C
    p1, p2 = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    off = np.array([[0, 0], [len(p1), len(p2)]], np.int64)
    T0, out = np.ascontiguousarray(np.asarray(init).reshape(16)), np.zeros(16)
    vs, rd, it = np.array(good[0], np.float64), np.array(good[1], np.float64), np.array(good[2], np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def call(v=vs, r=rd, i=it, nr=None, estimate=1, flags=0, L=2):
        return eng._lib.alignnet_icp_multiscale_register(eng._h, fp(p1), fp(p2), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, dp(T0), L, dp(v), dp(r), ip(i),
                                                         dp(nr), estimate, flags, dp(out), None, None, None, None)

    assert call() == 0
    assert np.array_equal(out.reshape(4, 4), before["transforms"][0])
    for kw, msg in ((dict(v=None), "null"), (dict(r=None), "null"), (dict(i=None), "null"), (dict(estimate=2), "null normal_radii"), (dict(estimate=3), "estimate"),
                    (dict(estimate=0), "estimate"), (dict(flags=2), "unknown flags"), (dict(L=0), "L must be"), (dict(L=9), "L must be")):
        rc = call(**kw)
        assert rc != 0
        with pytest.raises(EngineError, match=msg):
            eng._check(rc)
    with pytest.raises(EngineError):
        alignnet3d.Engine.icp_multiscale_refine_rows(eng, [10 ** 6], [init], *good)          # a row out of range (or no dataset)
    assert eng.get_option("icp_multiscale_ws_bytes") == used       # nothing was carved, nothing launched
    after = eng.icp_multiscale_refine([src], [dst], [init], *good)
    assert all(np.array_equal(before[k], after[k]) for k in before)


# ---- 5. the drop-in --------------------------------------------------------------------------------------------------------------------------------
# (the last level stays downsampled: these sources are subsets of their targets, so any schedule that ends on the raw clouds at radius 0.1 lands on
# the single-scale call's fixed point -- one closed-form step from anywhere near it -- and writes the same float32 files)
SCHEDULE = {"voxel_sizes": [0.6, 0.3], "radii": [0.6, 0.3], "its": [5, 5]}


def _val_call(val, inits, schedule):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    srcs, dsts = [v[0] for v in val], [v[1] for v in val]
    if schedule is None:
        T = e.icp_refine(srcs, dsts, inits, radius=0.1, its=30)["transforms"]
    else:
        T = e.icp_multiscale_refine(srcs, dsts, inits, schedule["voxel_sizes"], schedule["radii"], schedule["its"])["transforms"]
    e.close()
    return T


def test_train_py_icp_mode_multiscale(gpu_required, tmp_path):
    """The ICP baseline mode: with evaluation.icp_multiscale the files are those of Engine.icp_multiscale_refine on the same pairs from the centroid
    start; absent or false they are the single-scale call's."""
    sys.path.insert(0, PKG)
    import evaluation as EV
    root = tmp_path / "SynthTiny"
    val = _make_dataset(str(root))
    ev = tmp_path / "logs" / "icp_SynthTiny" / "icp_SynthTiny_o3_p2p" / "val" / "eval000000"
    cfgp = tmp_path / "icp_SynthTiny_o3_p2p.json"
    off = np.zeros((len(val) + 1, 2), np.int64)
    off[1:, 0], off[1:, 1] = np.cumsum([len(v[0]) for v in val]), np.cumsum([len(v[1]) for v in val])
    inits = alignnet3d.Engine.centroid_inits(np.concatenate([v[0] for v in val]), np.concatenate([v[1] for v in val]), off, range(len(val)))
    got = {}
    for name, evaluation in (("absent", {}), ("false", {"icp_multiscale": False}), ("multiscale", {"icp_multiscale": SCHEDULE})):
        json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
                   "evaluation": dict(evaluation, special={"mode": "icp", "icp": {"variant": "p2point", "with_constraint": True}})}, open(cfgp, "w"))
        out = _run(["train", "--config", str(cfgp)], str(tmp_path))
        assert ("ICP multi-scale" in out) == (name == "multiscale"), out[-2000:]
        got[name] = {k: np.load(ev / ("%s.npy" % k)) for k in ("pred_translations", "pred_angles")}
    for name, schedule in (("absent", None), ("false", None), ("multiscale", SCHEDULE)):
        T = _val_call(val, inits, schedule)
        assert np.array_equal(got[name]["pred_translations"], T[:, :3, 3].astype(np.float32)), name
        assert np.array_equal(got[name]["pred_angles"][:, 0], EV.rotvec_z(T[:, :3, :3]).astype(np.float32)), name
    assert not np.array_equal(got["multiscale"]["pred_translations"], got["absent"]["pred_translations"])


def test_train_py_refine_icp_multiscale(gpu_required, tmp_path):
    """--refineICP from stored predictions: with the key the refined files are the multi-scale call's, without it the single-scale call's."""
    sys.path.insert(0, PKG)
    import evaluation as EV
    root = tmp_path / "SynthTiny"
    val = _make_dataset(str(root))
    user = {"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")},
            "model": {"num_points": 64, "angles": {"num_bins": 12, "accept_inverted_angle": True},
                      "options": {"s1transformer": [[32, 64, 96], [[64, 32], 0.7]], "s2transformer": [[32, 64, 128], [[64, 32], 0.7]],
                                  "embedding": [32, 64, 160], "remaining_transform_prediction": [[64, 32], 0.7]}},
            "training": {"batch_size": 4, "num_epochs": 2, "learning_rate": 0.002}}
    cfgp = tmp_path / "MsRun.json"
    json.dump(user, open(cfgp, "w"))
    _run(["train", "--config", str(cfgp)], str(tmp_path))
    base = tmp_path / "logs" / "MsRun" / "val" / "eval000001"
    rng = np.random.default_rng(8)
    truth = np.stack([v[3] for v in val])
    stored_t = (truth[:, :3, 3] + rng.normal(0, 0.05, (len(val), 3))).astype(np.float32)
    stored_a = (np.arctan2(truth[:, 1, 0], truth[:, 0, 0]) + rng.normal(0, 0.03, len(val))).astype(np.float32).reshape(-1, 1)
    np.save(base / "pred_translations.npy", stored_t)
    np.save(base / "pred_angles.npy", stored_a)
    np.save(base / "pred_s2_pc1centers.npy", np.zeros((len(val), 3), np.float32))
    inits = [EV.get_mat_angle(stored_t[i], stored_a[i, 0], rotation_center=np.zeros(3, np.float32)) for i in range(len(val))]
    got = {}
    for name, evaluation in (("absent", {}), ("multiscale", {"icp_multiscale": SCHEDULE})):
        json.dump(dict(user, evaluation=evaluation), open(cfgp, "w"))
        out = _run(["eval_only", "--config", str(cfgp), "--eval_epoch", "1", "--refineICP", "--use_old_results"], str(tmp_path))
        assert ("ICP multi-scale" in out) == (name == "multiscale"), out[-2000:]
        got[name] = {k: np.load(base / "refined_p2p" / ("%s.npy" % k)) for k in ("pred_translations", "pred_angles")}
    for name, schedule in (("absent", None), ("multiscale", SCHEDULE)):
        T = _val_call(val, inits, schedule)
        assert np.array_equal(got[name]["pred_translations"], T[:, :3, 3].astype(np.float32)), name
        assert np.array_equal(got[name]["pred_angles"][:, 0], np.arctan2(T[:, 1, 0], T[:, 0, 0]).astype(got[name]["pred_angles"].dtype)), name
    assert not np.array_equal(got["multiscale"]["pred_translations"], got["absent"]["pred_translations"])
