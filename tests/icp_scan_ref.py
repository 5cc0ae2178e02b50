"""Inputs and fp64 margins for the tests of the ICP kernel's nearest-neighbour scan (csrc/alignnet_icp.hip: one fp32 pass per lane, an error bound
deciding per lane between none / single / walk, an fp64 tail behind the LDS stage, the quad's merge) -- tests/test_icp_scan_cpu.py and
tests/test_icp_scan_gpu.py.  TEST INFRASTRUCTURE ONLY; all arithmetic here is NumPy fp64, the loop and the estimates are oracle/icp_ref.py's and
tests/icp_full_ref.py's.

Two bounds, from standard rounding analysis (u64 = 2^-53, u32 = 2^-24; a sum of k rounded terms carries a relative error <= k u to first order):

b64(P, d) -- how far two CORRECT fp64 evaluations of |T p - q|^2 may differ (the kernel may fuse multiply-adds, NumPy does not; either is correct).
  A coordinate of T p = r . s + t is three products and three sums of terms whose magnitudes add up to at most P := max_i (|R| |s| + |t|)_i, so
  any evaluation order, fused or not, lands within 4 u64 P of the exact value; two evaluations differ by <= 8 u64 P per coordinate, i.e. by
  |delta| <= 8 sqrt(3) u64 P as a vector.  |p + delta - q|^2 - |p - q|^2 = 2 (p - q) . delta + |delta|^2 <= 2 sqrt(d) |delta| + |delta|^2.  Behind
  that, each evaluation rounds the three differences (relative u64 each: 2 u64 d on the sum of squares), the three squares and the two sums (3 u64 d
  more): 5 u64 d per evaluation, 10 u64 d between two.  So
      b64(P, d) = u64 (16 sqrt(3) P sqrt(d) + 10 d) + (8 sqrt(3) u64 P)^2.
  A source point whose gap between its two smallest DISTINCT distances, or whose distance to radius^2, is below UNDECIDED x b64 is undecided and left
  out of per-point comparisons; a pair with an undecided point in any evaluation is left out of whole-run comparisons.  Equal distances are decided by
  the index rule (lowest index), not undecided: identical target points give bit-identical distances in any one evaluation order.

need32(P, d) = u32 (2 sqrt(3) P sqrt(d) + 5 d) -- the error an fp32 evaluation of the same distance can really have (P := max |coordinate| of T p):
  the transformed point is rounded to fp32 (u32 P per coordinate, sqrt(3) u32 P as a vector: 2 sqrt(d) sqrt(3) u32 P on the squared distance) and
  the differences, squares and sums round as above (5 u32 d).  Used only to CLASSIFY inputs (is this a pair fp32 cannot resolve?), never as the
  kernel's threshold: what the tests ask of the kernel is stated for any sound certificate.
"""
import numpy as np

from oracle.icp_ref import _estimate_z
from tests.icp_full_ref import estimate_full, rot3

U32, U64, SQRT3 = 2.0 ** -24, 2.0 ** -53, np.sqrt(3.0)
UNDECIDED = 1000.0        # x b64
POINT_CAP = 1e-3          # share of a test's source points that may be undecided
LDS_BUDGET = 4266         # targets the kernel stages in LDS (150 KiB / 36 bytes)


def b64(P, d):
    return U64 * (16.0 * SQRT3 * P * np.sqrt(d) + 10.0 * d) + (8.0 * SQRT3 * U64 * P) ** 2


def need32(P, d):
    return U32 * (2.0 * SQRT3 * P * np.sqrt(d) + 5.0 * d)


def evaluate_with_margins(src, dst, T, radius, exact=False, rows=1 << 21):
    """One correspondence step in fp64, oracle/icp_ref.py::_evaluate's arithmetic (p = src R^T + t; ((dx^2 + dy^2) + dz^2); argmin = first index), with
    margins.  exact=True: the caller vouches that every operation is exact on this input (dyadic coordinates, identity T; the CPU test checks it in
    integers), so nothing is undecided.  Returns a dict of [n1] arrays: index, best, second (smallest distance > best, inf if none), gap, inlier,
    radius_margin |best - radius^2|, P64 / P32 (the magnitudes b64 / need32 take), undecided; plus fitness, rmse, p (transformed points)."""
    src, dst, T = np.asarray(src, np.float64)[:, :3], np.asarray(dst, np.float64)[:, :3], np.asarray(T, np.float64)
    n1, n2 = len(src), len(dst)
    p = src @ T[:3, :3].T + T[:3, 3]
    index, best, second = np.zeros(n1, np.int64), np.full(n1, np.inf), np.full(n1, np.inf)
    step = max(1, rows // max(n2, 1))
    for lo in range(0, n1, step):
        c = p[lo:lo + step]
        d2 = (c[:, 0:1] - dst[None, :, 0]) ** 2
        d2 += (c[:, 1:2] - dst[None, :, 1]) ** 2
        d2 += (c[:, 2:3] - dst[None, :, 2]) ** 2
        j = d2.argmin(1)
        b = d2[np.arange(len(c)), j]
        d2[d2 == b[:, None]] = np.inf
        index[lo:lo + step], best[lo:lo + step], second[lo:lo + step] = j, b, d2.min(1)
    r2 = radius * radius
    inlier = best <= r2
    P64 = (np.abs(src) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])).max(1) if n1 else np.zeros(0)
    P32 = np.abs(p).max(1) if n1 else np.zeros(0)
    gap, rm = second - best, np.abs(best - r2)
    und = np.zeros(n1, bool) if exact else (gap < UNDECIDED * b64(P64, np.where(np.isfinite(second), second, best))) | (rm < UNDECIDED * b64(P64, best))
    n = int(inlier.sum())
    return dict(index=index, best=best, second=second, gap=gap, inlier=inlier, radius_margin=rm, P64=P64, P32=P32, undecided=und, p=p,
                fitness=n / float(n1) if n1 else 0.0, rmse=float(np.sqrt(best[inlier].sum() / n)) if n else 0.0)


def icp_with_margins(src, dst, init, radius, its, constrained, info=None):
    """tests/icp_full_ref.py::icp_p2point's loop on evaluate_with_margins.  Returns (T, fitness, rmse, iterations, undecided points over all evaluations,
    evaluations).  info (a dict) receives `rank2`: the smallest ratio of the second to the first singular value of a non-zero centred cross-covariance
    over the estimates -- about 0 when the correspondences were collinear (two points; every source point on one of two targets), where a full 3-D
    rotation is not determined (the turn about the line is free) and no two SVDs need agree.  A ZERO covariance is not counted: both sides keep the rotation."""
    estimate = _estimate_z if constrained else estimate_full
    src, dst = np.asarray(src, np.float64)[:, :3], np.asarray(dst, np.float64)[:, :3]
    T = np.array(init, np.float64)
    if info is not None:
        info["rank2"] = np.inf
    if len(src) == 0 or len(dst) == 0:
        return T, 0.0, 0.0, 0, 0, 0
    e = evaluate_with_margins(src, dst, T, radius)
    und, k = int(e["undecided"].sum()), 0
    fit, rmse = e["fitness"], e["rmse"]
    rank2 = np.inf
    for k in range(1, its + 1):
        pp, qq = e["p"][e["inlier"]], dst[e["index"][e["inlier"]]]
        if len(pp):
            sv = np.linalg.svd((qq - qq.mean(0)).T @ (pp - pp.mean(0)), compute_uv=False)
            if sv[0] > 0:
                rank2 = min(rank2, sv[1] / sv[0])
        T = estimate(pp, qq) @ T
        e = evaluate_with_margins(src, dst, T, radius)
        und += int(e["undecided"].sum())
        done = abs(e["fitness"] - fit) < 1e-6 and abs(e["rmse"] - rmse) < 1e-6
        fit, rmse = e["fitness"], e["rmse"]
        if done:
            break
    if info is not None:
        info["rank2"] = rank2
    return T, fit, rmse, k, und, k + 1


def fp32_argmin(src, dst, T):
    """What a plain float32 scan would choose: the transformed point rounded to float32, float32 differences, squares and sums."""
    src, T = np.asarray(src, np.float64)[:, :3], np.asarray(T, np.float64)
    p = (src @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    q = np.asarray(dst, np.float32)[:, :3]
    out = np.zeros(len(p), np.int64)
    step = max(1, (1 << 21) // max(len(q), 1))
    for lo in range(0, len(p), step):
        c = p[lo:lo + step]
        d2 = (c[:, 0:1] - q[None, :, 0]) ** 2
        d2 += (c[:, 1:2] - q[None, :, 1]) ** 2
        d2 += (c[:, 2:3] - q[None, :, 2]) ** 2
        out[lo:lo + step] = d2.argmin(1)
    return out


def rigid_about(centre, angles, shift):
    """4x4: rotation rot3(*angles) about `centre`, then `shift`."""
    c = np.asarray(centre, np.float64)
    T = np.eye(4)
    T[:3, :3] = rot3(*angles)
    T[:3, 3] = c + np.asarray(shift, np.float64) - T[:3, :3] @ c
    return T


# ---- a. dense clouds far from the origin ----------------------------------------------------------------------------------------------------
SHAPES = ("cube", "sheet", "lines")
OFFSETS = (0.0, 50.0, 512.0, 4096.0, (-4096.0, 512.0, 30.0))


def dense_pair(shape, n2, offset, general, seed):
    """A dense target cloud `offset` metres from the origin and a 70 % subset of it with 0.5 mm of noise as the source.  cube: uniform in a 5 cm cube;
    sheet: a gently curved 25 x 25 cm sheet; lines: scan lines 5 cm apart, neighbours 2 - 5 mm apart along a line.  general=False: the source is
    the noisy subset itself and T the identity; True: the source is moved by the inverse of a general rigid motion T (tilts up to 0.1 rad about the
    cloud's centre, 3 cm of shift).  Returns (src, dst, T, init): T for one evaluation, init = T disturbed by 3 mm / 3 mrad (a point spacing) for whole runs."""
    rng = np.random.default_rng(seed)
    if shape == "cube":
        q = rng.uniform(0, 0.05, (n2, 3))
    elif shape == "sheet":
        xy = rng.uniform(0, 0.25, (n2, 2))
        q = np.concatenate([xy, 0.4 * (xy[:, :1] - 0.1) * (xy[:, 1:] - 0.15) + 0.3 * xy[:, :1] ** 2], 1)
    else:
        nl = 8
        per = -(-n2 // nl)
        x = np.cumsum(rng.uniform(0.002, 0.005, (nl, per)), 1)
        y = np.arange(nl)[:, None] * 0.05 + 0 * x
        q = np.stack([x, y, 0.05 * np.sin(2.0 * x + y * 7.0)], -1).reshape(-1, 3)[rng.permutation(nl * per)[:n2]]
    off = np.broadcast_to(np.asarray(offset, np.float64), (3,))
    dst = (q + off).astype(np.float32)
    keep = rng.permutation(n2)[: int(n2 * 0.7)]
    noisy = dst[keep].astype(np.float64) + rng.normal(0, 0.0005, (len(keep), 3))
    centre = dst.astype(np.float64).mean(0)
    if general:
        T = rigid_about(centre, rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.03, 0.03, 3))
        Ti = np.linalg.inv(T)
        src = (noisy @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    else:
        T, src = np.eye(4), noisy.astype(np.float32)
    init = rigid_about(centre, rng.normal(0, 3e-3, 3), rng.normal(0, 3e-3, 3)) @ T
    return src, dst, T, init


DENSE_SEED = 1
WHOLE_SEED = 2            # (seed 1 leaves one undecided point in one of the 60 whole runs: tests/test_icp_scan_cpu.py asserts none)
WHOLE_RUN = (("cube", 4000), ("sheet", 4566), ("lines", 4000))     # the pairs of the whole-run tests, per offset (general T)


def dense_cases():
    """Every (shape, n2, offset, general) of the per-point tests."""
    return [(sh, n2, off, gen) for sh in SHAPES for n2 in (4000, 4566) for off in OFFSETS for gen in (False, True)]


def offset_norm(offset):
    return float(np.abs(np.broadcast_to(np.asarray(offset, np.float64), (3,))).max())


# ---- b. planted near-ties --------------------------------------------------------------------------------------------------------------------
PLANT_RADIUS, PLANT_LDS, PLANT_TAIL = 0.05, 1024, 400
PLANT_CATEGORIES = ("same_slice", "cross_slice", "lds_tail", "both_tail")
PLANT_R = ("zero", "mid", "inside", "outside")
PLANT_PER = 40            # source points per (category, nearer-at-lower / -higher index)


def planted_pair(offset, seed):
    """320 source points, each with TWO targets at nearly equal fp64 distances, among fillers no nearer than 0.25 m, evaluated at a general rigid T (so
    that T p has fp64 granularity).  Per (category, order) PLANT_PER points, their distance class cycling over PLANT_R: `zero` = the nearer target is the
    float32 rounding of T p itself (the float32 scan sees distance 0: the floor of any threshold) and the farther its float32 neighbour on the far
    side of T p; `mid` = 2 cm; `inside` / `outside` = both targets just inside / just outside PLANT_RADIUS (by half of need32 on the squared
    distance).  Candidates are drawn, rounded to float32 and KEPT when the realised gap (fp64, after rounding) lies in [UNDECIDED b64, need32 / 8]
    ([.., need32] for `zero`, whose gap is of the size of its distances); kept gaps are thinned to spread log-uniformly over the band.  Target indices
    are placed per category: both in one lane's slice (equal mod 4, both LDS-resident), in different slices, one LDS-resident and one in the tail,
    both in the tail -- with lds_points = PLANT_LDS passed to the read-back.  Returns (src, dst, T, plan): plan = dict of [320] arrays category,
    order (0: nearer at the lower index), rclass, near, far (target indices), gap."""
    rng = np.random.default_rng(seed)
    off = np.broadcast_to(np.asarray(offset, np.float64), (3,))
    npl = len(PLANT_CATEGORIES) * 2 * PLANT_PER
    n2 = PLANT_LDS + PLANT_TAIL
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    sites = g[rng.permutation(len(g))[:npl]] - [3.5, 3.5, 2.0] + rng.uniform(-0.1, 0.1, (npl, 3)) + off
    T = rigid_about(off, rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.03, 0.03, 3))
    Ti = np.linalg.inv(T)
    src = (sites @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    p = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]                     # the restatement's T p
    P64 = (np.abs(src.astype(np.float64)) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])).max(1)
    P32 = np.abs(p).max(1)
    rclass = np.arange(npl) % len(PLANT_R)
    near, far, gaps = np.zeros((npl, 3), np.float32), np.zeros((npl, 3), np.float32), np.zeros(npl)
    R = PLANT_RADIUS
    for k in range(npl):
        name = PLANT_R[rclass[k]]
        m = 20000
        if name == "zero":
            a = np.tile(p[k].astype(np.float32), (3, 1))                   # (three candidates: the neighbour along each axis)
            b = a.copy()
            for ax in range(3):
                b[ax, ax] = np.nextafter(a[ax, ax], np.float32(np.inf if p[k, ax] > a[ax, ax] else -np.inf))
        else:
            r = {"mid": 0.02, "inside": R - need32(P32[k], R * R) / (4 * R), "outside": R + need32(P32[k], R * R) / (4 * R)}[name]
            u = rng.normal(size=(2, m, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
            a, b = (p[k] + r * u[0]).astype(np.float32), (p[k] + r * u[1]).astype(np.float32)
        da, db = ((p[k] - a.astype(np.float64)) ** 2).sum(1), ((p[k] - b.astype(np.float64)) ** 2).sum(1)
        swap = db < da
        a[swap], b[swap] = b[swap].copy(), a[swap].copy()
        da, db = np.minimum(da, db), np.maximum(da, db)
        gap = db - da
        lo, hi = UNDECIDED * b64(P64[k], db), need32(P32[k], db) / (1.0 if name == "zero" else 8.0)
        ok = (gap >= lo) & (gap <= hi)
        if name == "inside":
            ok &= db < R * R - UNDECIDED * b64(P64[k], db)
        if name == "outside":
            ok &= da > R * R + UNDECIDED * b64(P64[k], db)
        assert ok.any(), (k, name)
        cand = np.flatnonzero(ok)
        if name != "zero":   # log-uniform over the band: the kept candidate whose gap is nearest (in log) to a log-uniform draw
            want = np.exp(rng.uniform(np.log(lo[cand].min()), np.log(hi[cand].max())))
            cand = cand[[np.abs(np.log(gap[cand]) - np.log(want)).argmin()]]
        c = cand[0] if name != "zero" else cand[gap[cand].argmin()]
        near[k], far[k], gaps[k] = a[c], b[c], gap[c]
    # index placement
    free = {"lds": [list(rng.permutation(np.arange(s, PLANT_LDS, 4))) for s in range(4)], "tail": list(rng.permutation(np.arange(PLANT_LDS, n2)))}
    dst = np.zeros((n2, 3), np.float32)
    used = np.zeros(n2, bool)
    cat, order = np.repeat(np.arange(len(PLANT_CATEGORIES)), 2 * PLANT_PER), np.tile(np.repeat([0, 1], PLANT_PER), len(PLANT_CATEGORIES))
    ni, fi = np.zeros(npl, np.int64), np.zeros(npl, np.int64)
    for k in range(npl):
        s = int(rng.integers(4))
        if cat[k] == 0:
            i, j = free["lds"][s].pop(), free["lds"][s].pop()
        elif cat[k] == 1:
            i, j = free["lds"][s].pop(), free["lds"][(s + 1 + int(rng.integers(3))) % 4].pop()
        elif cat[k] == 2:
            i, j = free["lds"][s].pop(), free["tail"].pop()
        else:
            i, j = free["tail"].pop(), free["tail"].pop()
        i, j = (min(i, j), max(i, j))
        ni[k], fi[k] = (i, j) if order[k] == 0 else (j, i)
        dst[ni[k]], dst[fi[k]] = near[k], far[k]
        used[ni[k]] = used[fi[k]] = True
    nf = int((~used).sum())
    gf = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    fill = np.concatenate([gf, gf[rng.integers(len(gf), size=max(nf - len(gf), 0))]])[:nf] - [4.0, 4.0, 2.5] + rng.uniform(-0.15, 0.15, (nf, 3)) + off
    dst[~used] = fill.astype(np.float32)
    return src, dst, T, dict(category=cat, order=order, rclass=rclass, near=ni, far=fi, gap=gaps)


MULTI_LAYOUTS = ("same_slice", "spread", "lds_tail")
MULTI_PER = 32            # source points per (number of targets, layout)


def planted_multi(offset, seed):
    """Like planted_pair with THREE and FOUR targets per source point, all at 2 cm and all within need32 / 8 of each other in squared distance (no fp32
    evaluation orders any two of them), consecutive distances no closer than UNDECIDED b64 (fp64 orders them all).  Per (3 or 4, layout) MULTI_PER
    points: `same_slice` = all in one lane's slice (that lane keeps only its two smallest fp32 distances: a third under the threshold must still make it
    walk); `spread` = one per slice over three / four slices (three / four lanes in the quad's merge); `lds_tail` = two (LDS-resident, different
    slices) + one / two in the tail.  Which index holds the nearest is drawn at random.  Returns (src, dst, T, plan): plan = dict of m [n], layout [n],
    idx [n, 4] the planted targets' indices by ascending distance (-1 beyond m), span [n] largest - smallest squared distance."""
    rng = np.random.default_rng(seed)
    off = np.broadcast_to(np.asarray(offset, np.float64), (3,))
    npl = 2 * len(MULTI_LAYOUTS) * MULTI_PER
    n2 = PLANT_LDS + PLANT_TAIL
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    sites = g[rng.permutation(len(g))[:npl]] - [3.5, 3.5, 2.0] + rng.uniform(-0.1, 0.1, (npl, 3)) + off
    T = rigid_about(off, rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.03, 0.03, 3))
    Ti = np.linalg.inv(T)
    src = (sites @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    p = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    P64 = (np.abs(src.astype(np.float64)) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])).max(1)
    P32 = np.abs(p).max(1)
    ms = np.repeat([3, 4], len(MULTI_LAYOUTS) * MULTI_PER)
    layout = np.tile(np.repeat(np.arange(len(MULTI_LAYOUTS)), MULTI_PER), 2)
    free = {"lds": [list(rng.permutation(np.arange(s, PLANT_LDS, 4))) for s in range(4)], "tail": list(rng.permutation(np.arange(PLANT_LDS, n2)))}
    dst, used = np.zeros((n2, 3), np.float32), np.zeros(n2, bool)
    idx, span = np.full((npl, 4), -1, np.int64), np.zeros(npl)
    for k in range(npl):
        m = int(ms[k])
        u = rng.normal(size=(m, 40000, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
        q = (p[k] + 0.02 * u).astype(np.float32)
        d = np.sort(((p[k] - q.astype(np.float64)) ** 2).sum(-1), 0)                       # [m, draws], ascending per draw
        ok = (d[-1] - d[0] <= need32(P32[k], d[-1]) / 8) & (np.diff(d, axis=0).min(0) >= UNDECIDED * b64(P64[k], d[-1]))
        assert ok.any(), (k, m)
        c = np.flatnonzero(ok)[0]
        qs = q[:, c][np.argsort(((p[k] - q[:, c].astype(np.float64)) ** 2).sum(-1))]       # by ascending distance
        span[k] = d[-1, c] - d[0, c]
        s0 = int(rng.integers(4))
        if layout[k] == 0:
            slots = [free["lds"][s0].pop() for _ in range(m)]
        elif layout[k] == 1:
            slots = [free["lds"][(s0 + t) % 4].pop() for t in range(m)]
        else:
            slots = [free["lds"][s0].pop(), free["lds"][(s0 + 1) % 4].pop()] + [free["tail"].pop() for _ in range(m - 2)]
        slots = np.array(slots)[rng.permutation(m)]                                         # the nearest lands on any of them
        idx[k, :m] = slots
        dst[slots] = qs
        used[slots] = True
    nf = int((~used).sum())
    gf = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    fill = np.concatenate([gf, gf[rng.integers(len(gf), size=max(nf - len(gf), 0))]])[:nf] - [4.0, 4.0, 2.5] + rng.uniform(-0.15, 0.15, (nf, 3)) + off
    dst[~used] = fill.astype(np.float32)
    return src, dst, T, dict(m=ms, layout=layout, idx=idx, span=span)


# ---- c. radius edge --------------------------------------------------------------------------------------------------------------------------
def radius_edge_pair(radius):
    """Lattice target (spacing 2^-4, 6 x 6 x 4) and, beyond its +x face, source points at EXACTLY `radius` (2^-4 or 2^-3) from their only candidate
    (inliers: <=) followed by the same points one float32 ulp farther (not inliers).  Identity T: every operation is exact (dyadic coordinates)."""
    g = np.arange(6, dtype=np.float64) / 16.0
    lat = np.stack(np.meshgrid(g, g, g[:4], indexing="ij"), -1).reshape(-1, 3)
    lat = lat[np.random.default_rng(11).permutation(len(lat))]
    face = lat[lat[:, 0] == g[-1]]
    on = (face + [radius, 0.0, 0.0]).astype(np.float32)
    out = on.copy()
    out[:, 0] = np.nextafter(on[:, 0], np.float32(np.inf))
    return np.concatenate([on, out]), lat.astype(np.float32), np.eye(4), len(on)


# ---- d. size edges ---------------------------------------------------------------------------------------------------------------------------
SIZES_N1 = (1, 2, 3, 255, 256, 257, 512, 513)
SIZES_N2 = (1, 2, 3, 4, 5, 7, 8, 4265, 4266, 4267, 4269, 4270, 8533)


def size_pair(n1, n2, seed, duplicates=True):
    """n2 targets at a spacing of about 0.2 m; n1 source points = targets drawn at random + 2 cm of noise, moved by the inverse of a small z motion.
    Beyond the LDS budget, `duplicates` copies 40 LDS-resident targets into the tail and 40 tail targets into LDS slots (exact ties across the LDS /
    tail border: the lower index must win) and the first source points sit on those.  Returns (src, dst, init)."""
    rng = np.random.default_rng(seed)
    side = 0.2 * max(n2, 1) ** (1.0 / 3.0)
    dst = (rng.uniform(0, side, (n2, 3)) + rng.uniform(-5, 5, 3)).astype(np.float32)
    picks = rng.integers(n2, size=n1)
    noise = np.full((n1, 1), 0.02)
    if duplicates and n2 > LDS_BUDGET + 1:
        m = min(40, n2 - LDS_BUDGET)
        a, b = rng.permutation(LDS_BUDGET)[: 2 * m], LDS_BUDGET + rng.permutation(n2 - LDS_BUDGET)[:m]
        dst[b] = dst[a[:m]]                      # LDS-resident targets duplicated in the tail
        extra = LDS_BUDGET + rng.permutation(n2 - LDS_BUDGET)
        extra = extra[~np.isin(extra, b)][:m]
        dst[a[m: m + len(extra)]] = dst[extra]   # tail targets duplicated in LDS slots
        first = np.concatenate([b, extra])[:n1]
        picks[: len(first)] = first
        noise[: len(first)] = 0.001              # (these sit ON their duplicated target: the tie is between the two copies)
    th, t = rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02, 3)
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    src = ((dst[picks].astype(np.float64) + rng.normal(0, 1.0, (n1, 3)) * noise - t) @ Rz).astype(np.float32)
    init = np.eye(4); init[:3, :3] = Rz; init[:3, 3] = t
    return src, dst, init


BATCH_COLLINEAR = 66      # pairs of batch_pairs() whose correspondences are collinear (rank-1 cross-covariance): tests/test_icp_scan_cpu.py counts them


def batch_pairs(n_pairs=300, seed=77):
    """Heterogeneous pairs for one call: sizes cycling through SIZES_N1 x SIZES_N2 out of step, empty sources / targets in the middle, exactly one
    pair beyond the LDS budget among the first hundred (more would only repeat it).  Returns (srcs, dsts, inits)."""
    srcs, dsts, inits = [], [], []
    small = [n for n in SIZES_N2 if n <= 8] + [300, 511, 700]
    for k in range(n_pairs):
        n1 = SIZES_N1[k % len(SIZES_N1)]
        n2 = 4270 if k == 57 else small[(k * 7) % len(small)]
        s, d, i = size_pair(n1, n2, seed + k)
        if k in (140, 141):
            s = np.zeros((0, 3), np.float32)
        if k in (141, 142):
            d = np.zeros((0, 3), np.float32)
        srcs.append(s); dsts.append(d); inits.append(i)
    return srcs, dsts, inits


# ---- e. estimate branches --------------------------------------------------------------------------------------------------------------------
def estimate_pair(kind, seed):
    """Targets on a jittered grid (spacing 0.3 m: with radius 0.1 the correspondence of every source point is its own target) and sources that put the
    full-rotation estimate on a branch: `mirror` = the target's mirror image about its mid plane z = c (a slab 6 cm thick: the cross-covariance has
    a negative determinant, Umeyama's D = diag(1, 1, -1)); `planar` = exactly planar correspondences (z = 0.5 on both sides: rank 2); `planar_noise`
    = the same + 1e-6 of noise.  The source is then moved by a small rigid motion; init = identity, its = 1: the result is estimate(correspondences of
    the first evaluation).  Extents 2.4 x 1.2 m: singular values well separated.  Returns (src, dst, init)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(9), np.arange(5), indexing="ij"), -1).reshape(-1, 2) * 0.3
    xy = g + rng.uniform(-0.05, 0.05, g.shape) + [3.0, -2.0]
    if kind == "mirror":
        z = 0.5 + rng.uniform(-0.03, 0.03, len(xy))
        dst = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
        p = dst.astype(np.float64); p[:, 2] = 1.0 - p[:, 2]
        M = rigid_about(p.mean(0), [0.004, -0.003, 0.01], [0.004, -0.003, 0.002])
        src = (p @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    else:
        dst = np.concatenate([xy, np.full((len(xy), 1), 0.5)], 1).astype(np.float32)
        M = rigid_about(dst.astype(np.float64).mean(0), [0.0, 0.0, 0.01], [0.004, -0.003, 0.0])    # in-plane: z stays 0.5 exactly
        p = dst.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        if kind == "planar_noise":
            p = p + rng.normal(0, 1e-6, p.shape)
        src = p.astype(np.float32)
    return src, dst, np.eye(4)
