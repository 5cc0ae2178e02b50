"""Restatement helpers of the BINNED cast of csrc/alignnet_scene.hip (alignnet_set_option "scene_cast"), shared by
tests/test_scene_bin_cpu.py and tests/test_scene_bin_gpu.py: the per-triangle form of tests/scene_ref.py's azimuth intervals, bounds on the
length of every tile's triangle list derived from them, and the inputs the existing cases do not hold (a window with empty tiles inside, a mesh of
more triangles than one pass of a workgroup).

The bounds.  A tile is 8 consecutive columns of the window, counted from its first column.  Its list must hold every triangle a ray of the
tile hits (LOWER: the distinct triangles a cast record reports among the tile's columns) and may hold no triangle whose azimuth interval,
dilated by 1.01 columns on both sides -- the dilation tests/test_scene_gpu.py allows the window itself -- stays clear of the tile (UPPER;
a triangle whose xy projection holds the z axis, or which spans half the circle, counts for every tile; a zero-area triangle for none)."""
import functools

import numpy as np

from tests import scene_cases as C
from tests import scene_ref as R

TILE = 8
FULL_TILES = (R.HRES + TILE - 1) // TILE      # 563


def triangle_intervals(P, faces, margin):
    """Per face of the posed vertices P: kind [T] (0 = zero area, reaches nothing; 1 = the whole columns ca .. cb; 2 = every column), ca, cb [T]
    int64 (unwrapped: take them modulo 4500).  tests/scene_ref.py window(), kept per triangle."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    T = len(f)
    if not T:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    N = R.triangle_setup(P, f)[0]
    a, b, d = P[f[:, 0], :2], P[f[:, 1], :2], P[f[:, 2], :2]
    cr = lambda p, q: p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]
    dot = lambda p, q: p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]
    o1, o2, o3 = cr(a, b), cr(b, d), cr(d, a)
    ext = np.maximum(np.maximum(np.abs(a).sum(1), np.abs(b).sum(1)), np.abs(d).sum(1))
    m = 1e-12 * ext * ext
    solid = np.abs(o1 + o2 + o3) > m
    inside = ((o1 >= -m) & (o2 >= -m) & (o3 >= -m)) | ((o1 <= m) & (o2 <= m) & (o3 <= m))
    across = np.minimum(np.minimum(dot(a, b), dot(b, d)), dot(d, a)) <= m
    full = np.where(solid, inside, across)
    col = lambda p: (np.arctan2(p[:, 0], p[:, 1]) * 57.29577951308232 + 180.0) * (R.HRES / 360.0)
    c0 = col(a)
    d1, d2 = col(b) - c0, col(d) - c0
    d1 -= R.HRES * np.rint(d1 / R.HRES); d2 -= R.HRES * np.rint(d2 / R.HRES)
    lo, hi = c0 + np.minimum(0.0, np.minimum(d1, d2)), c0 + np.maximum(0.0, np.maximum(d1, d2))
    full |= hi - lo >= R.HRES / 2 - 1.0
    kind = np.where(np.any(N != 0, 1), np.where(full, 2, 1), 0).astype(np.int64)
    return kind, np.floor(lo - margin).astype(np.int64), np.ceil(hi + margin).astype(np.int64)


def tiles_of(count):
    return (count + TILE - 1) // TILE


def upper_bound(P, faces, window, margin=1.01):
    """[tiles of the window]: the triangles whose interval, widened by `margin` columns, touches the tile."""
    first, count = window
    kind, ca, cb = triangle_intervals(P, faces, margin)
    cov = np.zeros((len(kind), R.HRES), bool)
    for i in np.flatnonzero(kind == 1):
        cov[i, np.arange(ca[i], cb[i] + 1) % R.HRES] = True
    cov[kind == 2] = True
    cov = cov[:, R.window_columns(first, count)]
    return np.array([int(cov[:, k * TILE:(k + 1) * TILE].any(1).sum()) for k in range(tiles_of(count))], np.int64)


def lower_bound(triangle, window):
    """[tiles of the window]: distinct triangles a record (triangle [64, 4500] by ray, -1 = miss) reports among the tile's columns."""
    first, count = window
    tri = np.asarray(triangle)[:, R.window_columns(first, count)]
    out = []
    for k in range(tiles_of(count)):
        t = tri[:, k * TILE:(k + 1) * TILE]
        out.append(len(np.unique(t[t >= 0])))
    return np.array(out, np.int64)


def _two_blobs():
    ev, ef = C.ellipsoid(1)
    v = np.concatenate([ev * 0.5 + [0, -2.5, 0], ev * 0.5 + [0, 2.5, 0]])
    f = np.concatenate([ef, ef + len(ev)]).astype(np.int32)
    return v, f, 1.0, C.polar(12.0, 57.0, yaw=0.3)


# two small ellipsoids 5 m apart seen side by side: one window, a run of tiles between them that no triangle reaches
EXTRA = {"two_blobs": _two_blobs()}


def case(name):
    return EXTRA[name] if name in EXTRA else C.CASES[name]


@functools.lru_cache(None)
def reference(name):
    """The restatement's cloud of a case (scene_cases.reference for its own names)."""
    if name in C.CASES:
        return C.reference(name)
    v, f, scale, pose = EXTRA[name]
    return R.cloud(v, f, scale, pose, tables=R.sensor_tables())


def record_by_ray(ref):
    """triangle [64, 4500] by ray index of a restatement cloud (the layout of Engine.debug_scene_cast)."""
    out = np.full((R.VRES, R.HRES), -1, np.int64)
    out[:, R.window_columns(*ref["window"])] = ref["cast"]["triangle"]
    return out


def case_bounds(name):
    """(lower, upper) per tile of the restatement's own window, the restatement's record standing for the device's."""
    v, f, scale, pose = case(name)
    ref = reference(name)
    return lower_bound(record_by_ray(ref), ref["window"]), upper_bound(ref["posed"], f, ref["window"])


def subdivide(v, f, target):
    """Midpoint subdivision (1 -> 4 triangles): whole passes while they stay under `target` faces, then the first faces one by one up to it
    (tools/scene_rate.py's)."""
    v = list(map(tuple, np.asarray(v, np.float64))); f = [tuple(int(i) for i in t) for t in f]
    while len(f) < target:
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                v.append(tuple((np.array(v[a]) + np.array(v[b])) / 2)); mid[k] = len(v) - 1
            return mid[k]
        split = len(f) if 4 * len(f) <= target else -(-(target - len(f)) // 3)
        for a, b, c in f[:split]:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf + f[split:]
    return np.array(v, np.float64), np.array(f, np.int32)


@functools.lru_cache(None)
def car2064():
    """The built-in car after one full midpoint subdivision: 2,064 triangles (more than one pass of a 256-thread workgroup, more than one LDS chunk)."""
    v, f = C.car()
    return subdivide(v, f, 4 * len(f))
