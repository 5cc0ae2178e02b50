"""Inputs and an fp64 restatement of the cell function for the tests of the ICP kernel's grid search (csrc/alignnet_icp.hip: icp_grid_build_kernel,
icp_kernel<kFull, kTrace, true>) -- tests/test_icp_grid_cpu.py and tests/test_icp_grid_gpu.py.  TEST INFRASTRUCTURE ONLY; all arithmetic here is NumPy
fp64.  The yardstick of every comparison is tests/icp_scan_ref.py (evaluate_with_margins, icp_with_margins, b64, UNDECIDED, POINT_CAP): the grid
search must choose what the brute-force restatement chooses.

The cell function, as the kernel states it: e = max(radius (1 + 2^-20), (M + radius) 2^-20) with M the largest |coordinate| of the pair's target;
cell(x) = clip(floor(x / e), -2^30, 2^30) per axis, in fp64 from the float32 coordinates (targets) or the fp64 transformed point (queries).  A query
evaluates the targets of the 27 cells around its own (and whatever else shares their hash buckets: more candidates, never fewer)."""
import functools

import numpy as np

from tests.icp_full_ref import rot3

SPAN = 2.0 ** -20
CELL_MAX = 2.0 ** 30
RADIUS = 0.1
BOX = (4.4, 1.8, 1.4)


def cell_edge(dst, radius, margin=True):
    """margin=False: e = radius exactly -- the cell width that LOSES inliers (tests/test_icp_grid_cpu.py shows it)."""
    if not margin:
        return float(radius)
    M = float(np.abs(np.asarray(dst, np.float64)).max()) if len(dst) else 0.0
    return max(radius * (1.0 + SPAN), (M + radius) * SPAN)


def cells(x, e):
    return np.clip(np.floor(np.asarray(x, np.float64) / e), -CELL_MAX, CELL_MAX).astype(np.int64)


def neighbour_counts(p, dst, e, radius, rows=1 << 21):
    """Per query p [n1, 3] (fp64): how many targets lie in its 27 cells, how many within `radius` (fp64 squared distance <= radius^2, the restatement's
    arithmetic), and how many of the latter are NOT in the 27 cells (must be 0)."""
    p, dst = np.asarray(p, np.float64), np.asarray(dst, np.float64)
    cq = cells(dst, e)
    near27, within, lost = np.zeros(len(p), np.int64), np.zeros(len(p), np.int64), np.zeros(len(p), np.int64)
    step = max(1, rows // max(len(dst), 1))
    for lo in range(0, len(p), step):
        c = p[lo:lo + step]
        cp = cells(c, e)
        n27 = (np.abs(cp[:, None, :] - cq[None, :, :]) <= 1).all(-1)
        d2 = (c[:, 0:1] - dst[None, :, 0]) ** 2
        d2 += (c[:, 1:2] - dst[None, :, 1]) ** 2
        d2 += (c[:, 2:3] - dst[None, :, 2]) ** 2
        w = d2 <= radius * radius
        near27[lo:lo + step], within[lo:lo + step], lost[lo:lo + step] = n27.sum(1), w.sum(1), (w & ~n27).sum(1)
    return near27, within, lost


# ---- a. the box-surface recipe ---------------------------------------------------------------------------------------------------------------
RECIPE_N2 = (4267, 6000)
RECIPE_OFFSETS = (0.0, 512.0, 4096.0)


def box_surface(rng, n):
    """n points on the faces of a BOX-sized box centred at the origin, 5 mm of roughness along the face normal."""
    dims = np.asarray(BOX)
    area = np.array([dims[1] * dims[2], dims[0] * dims[2], dims[0] * dims[1]])
    axis = rng.choice(3, size=n, p=area / area.sum())
    q = rng.uniform(-0.5, 0.5, (n, 3)) * dims
    side = rng.choice([-0.5, 0.5], size=n)
    q[np.arange(n), axis] = side * dims[axis] + rng.normal(0, 0.005, n)
    return q


@functools.lru_cache(maxsize=None)
def box_pair(n2, offset, seed=5):
    """Target: n2 float32 points on the box surface + a uniform(-15, 15) shift + `offset`.  Source: a 70 % subset moved by the inverse of a small 3-D
    motion (tilts <= 0.05 rad about the cloud's centre, <= 6 cm); a fifth of it pushed 0.05 - 0.2 m in random directions (some end inside, some
    outside the radius).  Returns (src, dst, T, init): T the motion source -> target, init = T disturbed by N(0, 0.01) in rotation and translation."""
    rng = np.random.default_rng(seed + 1000 * n2 + int(offset))
    dst = (box_surface(rng, n2) + rng.uniform(-15, 15, 3) + offset).astype(np.float32)
    keep = rng.permutation(n2)[: int(n2 * 0.7)]
    q = dst[keep].astype(np.float64)
    push = rng.permutation(len(q))[: len(q) // 5]
    u = rng.normal(size=(len(push), 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    q[push] += u * rng.uniform(0.05, 0.2, (len(push), 1))
    qc = dst.astype(np.float64).mean(0)
    R, t = rot3(*rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.06, 0.06, 3)
    src = ((q - qc - t) @ R + qc).astype(np.float32)                      # q - qc = R (p - qc) + t
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = qc + t - R @ qc
    E = np.eye(4); E[:3, :3] = rot3(*rng.normal(0, 0.01, 3)); E[:3, 3] = qc + rng.normal(0, 0.01, 3) - E[:3, :3] @ qc
    for a in (src, dst, T):
        a.setflags(write=False)
    init = E @ T
    init.setflags(write=False)
    return src, dst, T, init


# ---- b. exact ties and the radius on a cell border --------------------------------------------------------------------------------------------
TIE_RADIUS = 2.0 ** -3
TIE_SPACING = 2.0 ** -4


def tie_pair(offset, seed=9):
    """Target: a 17^3 lattice of spacing 2^-4 in shuffled index order at `offset` (+ lone targets, below).  Identity T, dyadic coordinates: every
    operation of the distance is exact.  Sources: midpoints of lattice edges, faces and cells (2, 4 and 8 targets at the same distance: the lowest
    original index must win); and, for lone targets placed a step of 2^-10 below, on and above multiples of the cell edge along each axis, the six
    points EXACTLY one radius from them (inliers: <=; target and source then sit on different sides of a cell border for some of them).
    Returns (src, dst, kinds): kinds [n1] = 2 / 4 / 8 for the midpoints, 1 for the radius points."""
    rng = np.random.default_rng(seed)
    g = np.arange(17, dtype=np.float64) * TIE_SPACING
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    e = TIE_RADIUS * (1.0 + SPAN)
    lone = []
    for k, axis in enumerate((0, 1, 2, 0, 1, 2)):
        base = np.array([4.0 + 2.0 * k, 0.5, 0.5])                        # 2 m apart, 3 m from the lattice: lone
        border = np.round((np.floor((offset + base[axis]) / e) + 1) * e * 1024.0) / 1024.0 - offset
        for step in (-1, 0, 1):
            t = base + [0.0, 0.25 * (step + 1), 0.0] if axis != 1 else base + [0.25 * (step + 1), 0.0, 0.0]
            t[axis] = border + step / 1024.0
            lone.append(t)
    lone = np.array(lone)
    dst = np.concatenate([lat, lone])
    perm = rng.permutation(len(dst))
    dst = dst[perm]
    i = rng.integers(0, 16, (120, 3)).astype(np.float64) * TIE_SPACING
    h = TIE_SPACING / 2
    mids, kinds = [], []
    for m, (shift, kind) in enumerate((([h, 0, 0], 2), ([0, h, 0], 2), ([0, 0, h], 2), ([h, h, 0], 4), ([0, h, h], 4), ([h, 0, h], 4), ([h, h, h], 8))):
        pts = i[m::7] + shift
        mids.append(pts); kinds += [kind] * len(pts)
    edge = np.concatenate([lone + s * TIE_RADIUS * np.eye(3)[a] for a in range(3) for s in (-1.0, 1.0)])
    src = np.concatenate(mids + [edge]) + offset
    kinds = np.array(kinds + [1] * len(edge))
    d32, s32 = (dst + offset).astype(np.float32), src.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), dst + offset) and np.array_equal(s32.astype(np.float64), src)   # dyadic: nothing rounded
    return s32, d32, kinds


# ---- c. a heavy bucket, a wide extent, a far start ---------------------------------------------------------------------------------------------
def heavy_pair(seed=21):
    """5,000 targets: 3,000 copies of ONE point (one bucket far over any typical size; every copy ties, the lowest index wins) among 2,000 on the box
    surface, shuffled.  Sources: 300 within 3 cm of the heavy point, 1,100 near surface points.  Returns (src, dst, init)."""
    rng = np.random.default_rng(seed)
    surf = box_surface(rng, 2000) + [3.0, -2.0, 1.0]
    heavy = surf[0] + [0.0, 0.0, 0.3]
    dst = np.concatenate([np.tile(heavy, (3000, 1)), surf])[rng.permutation(5000)].astype(np.float32)
    near = heavy + rng.normal(0, 0.01, (300, 3))
    q = np.concatenate([near, surf[rng.permutation(2000)[:1100]] + rng.normal(0, 0.003, (1100, 3))])
    qc = dst.astype(np.float64).mean(0)
    R, t = rot3(*rng.uniform(-0.02, 0.02, 3)), rng.uniform(-0.02, 0.02, 3)
    src = ((q - qc - t) @ R + qc).astype(np.float32)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = qc + t - R @ qc
    E = np.eye(4); E[:3, :3] = rot3(*rng.normal(0, 0.003, 3)); E[:3, 3] = qc + rng.normal(0, 0.003, 3) - E[:3, :3] @ qc
    return src, dst, E @ T


def cluster_pair(wide, seed=22):
    """4,501 targets: two box-surface clusters of 2,250 points (`wide`: 3 km apart; else 3 m apart) plus one stray point; the source samples both
    clusters.  Same n1 and n2 either way.  Returns (src, dst, init)."""
    rng = np.random.default_rng(seed)
    a, b = box_surface(rng, 2250), box_surface(rng, 2250) + ([3000.0, 0.0, 0.0] if wide else [0.0, 3.0, 0.0])
    stray = np.array([[-700.0, 40.0, 2.0]]) if wide else np.array([[0.0, -3.0, 2.0]])
    dst = np.concatenate([a, b, stray])[rng.permutation(4501)].astype(np.float32)
    q = np.concatenate([a[:1500], b[:1500]]) + rng.normal(0, 0.002, (3000, 3))
    th, t = 0.01, np.array([0.02, -0.01, 0.015])
    R = rot3(0.0, 0.0, th)
    src = ((q - t) @ R).astype(np.float32)                                # q = R p + t
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    E = np.eye(4); E[:3, 3] = [0.004, -0.003, 0.002]
    return src, dst, E @ T


# ---- d. size edges -----------------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def size_cases():
    """(n1, n2) drawn from SIZES, not the full product: every size once as n1 and once as n2 (out of step), plus both sides of the scan's LDS budget."""
    k = len(SIZES)
    return [(SIZES[i], SIZES[(i * 5 + 3) % k]) for i in range(k)] + [(257, 4266), (257, 4267), (1025, 4267)]
