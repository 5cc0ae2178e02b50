"""fp64 NumPy restatement of the BAND MASK of the cast by elevation band (alignnet_set_option "scene_rows", csrc/alignnet_scene.hip stage 2c),
shared by tests/test_scene_rows_cpu.py and tests/test_scene_rows_gpu.py.

A tile is 8 consecutive columns of a cloud's window, a band 8 consecutive rows, a cell a (tile, band).  A staged triangle is intersected with a
cell only when its mask has the band's bit.  The rule, from the posed vertices alone: a ray of column c and row r meets the triangle at P = t d,
t > 0, so dir_z[r] = n_c P.z / rho(P) with n_c = |(dir_x[c], dir_y[c])| and rho the distance from the z axis.  Over the triangle P.z lies between
the extreme vertex z and rho between rho_min -- the distance from the axis to the xy projection, the smallest of the three point-to-SEGMENT
distances -- and rho_max, the largest vertex rho; the signs of z_min and z_max say which bound goes with which, the range of n_c over the tile's
columns multiplies in, and bit b is set iff one of the band's eight dir_z values lies in the interval (the table need not be monotone).  Every
band is set when the xy projection holds the axis, when rho_min <= 1e-6 rho_max, or when the triangle's plane passes so close to the sensor (or the
triangle is such a sliver) that the kernel's rounded hit test can reach beyond the widened interval; a face of zero area gets no band.

margin widens s = z / rho by margin (1 + |s|) on both sides (the device's is 1e-8; 0 here tests the rule itself).  guard moves every threshold
of the every-band cases by that factor towards "every band" (1 = the device's), and > 1 does not exclude zero-area faces.  It is there for rounding
alone: a triangle within the device's rounding of a threshold may fall on either side of it there, so an UPPER bound on the device's masks takes
every band for it.  The compared quantities are a dozen fp64 operations each, good to 1e-15 of their scale (cancellation included: the side
products to 4e-16 ext^2 against the threshold 1e-12 ext^2), so UPPER_GUARD = 1.01 is thirteen orders above what rounding can move and still sends
no triangle to every band that is not within 1 % of a threshold.  vertex_only = True is the WRONG rule that takes rho_min from the vertices,
kept for the mutation test."""
import numpy as np

from tests import scene_bin_ref as BR
from tests import scene_ref as R

TILE, BAND, BANDS = 8, 8, R.VRES // 8
DEVICE_MARGIN, ETA = 1e-8, 2e-14
UPPER_MARGIN, UPPER_GUARD = 1e-5, 1.01      # the upper bound on the device's masks: the margin 1000 times the device's, the guard as above


def _seg_dist2(p, q):
    """Squared distance from the origin to the segments p .. q of the xy plane ([T, 2] each)."""
    e = q - p
    ee = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0, np.clip(-(p[:, 0] * e[:, 0] + p[:, 1] * e[:, 1]) / ee, 0.0, 1.0), 0.0)
    x, y = p[:, 0] + t * e[:, 0], p[:, 1] + t * e[:, 1]
    return x * x + y * y


def slope_intervals(P, faces, margin=0.0, guard=1.0, vertex_only=False):
    """Per face: kind [T] (0 = no band, 1 = the interval [s_lo, s_hi] of z / rho, 2 = every band), s_lo, s_hi [T]."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    T = len(f)
    if not T:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
    N, _, _, c = R.triangle_setup(P, f)
    A, B, D = P[f[:, 0]], P[f[:, 1]], P[f[:, 2]]
    a, b, d = A[:, :2], B[:, :2], D[:, :2]
    cr = lambda p, q: p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]
    dot = lambda p, q: p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]
    o1, o2, o3 = cr(a, b), cr(b, d), cr(d, a)
    ext = np.maximum(np.maximum(np.abs(a).sum(1), np.abs(b).sum(1)), np.abs(d).sum(1))
    m = 1e-12 * ext * ext
    mg = m * guard
    inside = ((o1 >= -mg) & (o2 >= -mg) & (o3 >= -mg)) | ((o1 <= mg) & (o2 <= mg) & (o3 <= mg))
    across = np.minimum(np.minimum(dot(a, b), dot(b, d)), dot(d, a)) <= mg
    area = np.abs(o1 + o2 + o3)
    full = ((area > m / guard) & inside) | ((area <= mg) & across)      # (guard = 1: np.where(area > m, inside, across), the device's branch)
    ra, rb, rd = dot(a, a), dot(b, b), dot(d, d)
    rmax2 = np.maximum(np.maximum(ra, rb), rd)
    rmin2 = np.minimum(np.minimum(ra, rb), rd) if vertex_only else np.minimum(np.minimum(_seg_dist2(a, b), _seg_dist2(b, d)), _seg_dist2(d, a))
    full |= ~(rmin2 > 1e-12 * guard * guard * rmax2)
    rmin, rmax = np.sqrt(rmin2), np.sqrt(rmax2)
    p2 = np.maximum(np.maximum(ra + A[:, 2] ** 2, rb + B[:, 2] ** 2), rd + D[:, 2] ** 2)
    e2 = np.maximum(np.maximum(((B - A) ** 2).sum(1), ((D - B) ** 2).sum(1)), ((A - D) ** 2).sum(1))
    g, ac = ETA * guard * p2, np.abs(c)
    with np.errstate(over="ignore", invalid="ignore"):
        full |= ~((g * g) * e2 < 0.25 * (ac * ac)) | ~(4.0 * (g * e2) < (DEVICE_MARGIN * rmin) * ac)
    zmin, zmax = np.minimum(np.minimum(A[:, 2], B[:, 2]), D[:, 2]), np.maximum(np.maximum(A[:, 2], B[:, 2]), D[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        s_lo = zmin / np.where(zmin >= 0, rmax, rmin)
        s_hi = zmax / np.where(zmax >= 0, rmin, rmax)
    s_lo = s_lo - margin * (1.0 + np.abs(s_lo))
    s_hi = s_hi + margin * (1.0 + np.abs(s_hi))
    kind = np.where(full, 2, 1)
    if guard <= 1:
        kind = np.where(np.any(N != 0, 1), kind, 0)
    return kind.astype(np.int64), s_lo, s_hi


def masks(P, faces, window, tables, margin=0.0, guard=1.0, vertex_only=False):
    """[tiles of the window, T] the 8-bit band mask of every face for every tile."""
    dx, dy, dz = tables
    first, count = window
    kind, s_lo, s_hi = slope_intervals(P, faces, margin, guard, vertex_only)
    cols = R.window_columns(first, count)
    out = np.zeros((BR.tiles_of(count), len(kind)), np.int64)
    for k in range(len(out)):
        n = np.sqrt(dx[cols[k * TILE:(k + 1) * TILE]] ** 2 + dy[cols[k * TILE:(k + 1) * TILE]] ** 2)
        with np.errstate(invalid="ignore"):
            lo = np.minimum(s_lo * n.min(), s_lo * n.max())
            hi = np.maximum(s_hi * n.min(), s_hi * n.max())
            rows = (lo[:, None] <= dz[None, :]) & (dz[None, :] <= hi[:, None])      # [T, 64]
        bands = rows.reshape(-1, BANDS, BAND).any(2)
        bands = np.where((kind == 2)[:, None], True, bands) & (kind != 0)[:, None]
        out[k] = (bands * (1 << np.arange(BANDS))).sum(1)
    return out


def missed(cast_triangle, mask):
    """The hit rays of a record on the window's own columns (triangle [64, count], -1 = miss) whose band is NOT in the mask of the triangle they
    hit for their tile: (row, window column, triangle) triples.  Sufficiency is `not missed`."""
    tri = np.asarray(cast_triangle)
    r, j = np.nonzero(tri >= 0)
    t = tri[r, j]
    bad = ((mask[j // TILE, t] >> (r // BAND)) & 1) == 0
    return list(zip(r[bad].tolist(), j[bad].tolist(), t[bad].tolist()))


def cell_lower(triangle, window):
    """[tiles, 8]: distinct triangles a record by ray index (triangle [64, 4500]) reports among the rays of every cell."""
    first, count = window
    tri = np.asarray(triangle)[:, R.window_columns(first, count)]
    out = np.zeros((BR.tiles_of(count), BANDS), np.int64)
    for k in range(len(out)):
        for b in range(BANDS):
            t = tri[b * BAND:(b + 1) * BAND, k * TILE:(k + 1) * TILE]
            out[k, b] = len(np.unique(t[t >= 0]))
    return out


def list_members(P, faces, window, margin=1.01):
    """[tiles, T] bool: the faces a tile's list may hold (tests/scene_bin_ref.py's upper bound, kept per face)."""
    first, count = window
    kind, ca, cb = BR.triangle_intervals(P, faces, margin)
    cov = np.zeros((len(kind), R.HRES), bool)
    for i in np.flatnonzero(kind == 1):
        cov[i, np.arange(ca[i], cb[i] + 1) % R.HRES] = True
    cov[kind == 2] = True
    cov = cov[:, R.window_columns(first, count)]
    return np.array([cov[:, k * TILE:(k + 1) * TILE].any(1) for k in range(BR.tiles_of(count))], bool).reshape(BR.tiles_of(count), len(kind))


def scan_members(P, faces, window, tables):
    """[tiles, T] bool: the faces the scan's staging may keep for a tile -- its two side tests restated with twice the margin on the keeping side
    (all three vertices strictly before the first column's half plane, or strictly behind the last one's, are culled)."""
    dx, dy, _ = tables
    first, count = window
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cols = R.window_columns(first, count)
    X, Y = P[f, 0], P[f, 1]                                            # [T, 3]
    m = 2.0 * 1e-12 * 120.0 * (np.abs(X) + np.abs(Y))
    out = np.zeros((BR.tiles_of(count), len(f)), bool)
    for k in range(len(out)):
        ca, cb = cols[k * TILE], cols[min((k + 1) * TILE, count) - 1]
        before = (dx[ca] * Y - dy[ca] * X > m).all(1)
        behind = (dx[cb] * Y - dy[cb] * X < -m).all(1)
        out[k] = ~before & ~behind
    return out


def cell_upper(members, mask):
    """[tiles, 8]: per cell, the faces among `members` [tiles, T] whose (loose) mask [tiles, T] has the band's bit."""
    return np.stack([(members & (((mask >> b) & 1) == 1)).sum(1) for b in range(BANDS)], 1).astype(np.int64)
