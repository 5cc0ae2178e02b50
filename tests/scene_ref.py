"""fp64 NumPy restatement of the spinning-LiDAR scene generator of csrc/alignnet_scene.hip (alignnet_scene_generate): the ray cast of
SyntheticScene.generate_pointcloud_embree (tp_utils/pointcloud.py:1119-1138) with the sensor of :945-971 and the meshes of :447-454.

TEST INFRASTRUCTURE ONLY, and UNPINNED where it has to be: trimesh and embree are not available next to this stack, so what a "hit" is
cannot be taken from them.  This file IS the definition the kernels are held to.

The reference's, restated:
  the sensor (64 x 4500 rays from the origin, idx = vidx * 4500 + hidx, direction 120 (sin h, cos h, tan v), unbounded in range);
  the posed mesh, world vertex = Rz(angle) (mesh_scale v) + position in fp64 on the normalised vertices;
  the first hit per ray, two-sided triangles, location = t d, the hits kept in ascending ray index (the 20 ray parts, concatenated);
  the noise strength max(0.005, sigma |centroid| / 80) with the area-weighted centroid of the posed mesh, the clip at +-clip.

This project's own:
  * the intersection test is the scalar-triple-product form of Moeller-Trumbore with the ray origin at 0.  Per triangle (v0, v1, v2),
    e1 = v1 - v0, e2 = v2 - v0:  N = e1 x e2,  A = e2 x v0,  Bv = v0 x e1,  c = v0 . N;  per ray d:  den = d . N,  u = (d . A) / den,
    v = (d . Bv) / den,  t = c / den;  a hit has den != 0, u >= 0, v >= 0, u + v <= 1 and t > 0; the smallest t wins, equal t going to the
    lower triangle index.  A zero-area triangle has N = 0 exactly (den = 0) and never hits.  Every product and sum is rounded once, in the
    order written (NumPy has no fused multiply-add; the kernel switches contraction off to match);
  * embree's watertightness rules at shared edges are not restated.  Instead every window is cast three ways -- plain (above), DILATED
    (u, v, 1 - u - v >= -1e-9, |den| / (|d| |N|) > 0) and ERODED (>= +1e-9, > 1e-9) -- and a ray on which dilated and eroded disagree (hit
    or miss, or t by more than 1e-9 m) is UNDECIDED: a test skips it, and allows at most 2 of them per cloud;
  * the azimuth window: a triangle covers the columns between the azimuths of its vertices (+- a margin), all 4500 when its xy
    projection holds the z axis; the window is the complement of the largest uncovered gap of the circle of columns (it may wrap);
  * the noise z is the dataset sampler's counter stream (oracle/dataset_ref.py: mix64 + Box-Muller, float32), keyed by
    (seed, scene id, cloud, ray index); it is NOT np.random.randn's stream, so generated clouds are distributed like the reference's,
    not equal to them; point = float32(location) + clip(strength z, +-clip) in float32.
"""
import numpy as np

from oracle.dataset_ref import mix64

VRES, VFOV, HRES, HFOV = 64, 26.9, 4500, 360.0
EPS = 1e-9
T_TOL = 1e-9


def sensor_tables():
    """pointcloud.py:957-971: (120 sin h [4500], 120 cos h [4500], 120 tan v [64])."""
    vangle = -VFOV / 2.0 + VFOV / (VRES - 1) * np.arange(VRES)
    hangle = -HFOV / 2.0 + HFOV / (HRES) * np.arange(HRES)
    return (np.sin(hangle / 180. * np.pi) * 120.0, np.cos(hangle / 180. * np.pi) * 120.0, np.tan(vangle / 180. * np.pi) * 120.0)


def pose_vertices(vertices, scale, pose):
    """Rz(angle) (scale v) + position; pose = (x, y, z, angle)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    c, s = np.cos(pose[3]), np.sin(pose[3])
    sx, sy, sz = scale * v[:, 0], scale * v[:, 1], scale * v[:, 2]
    return np.stack([(c * sx - s * sy) + pose[0], (s * sx + c * sy) + pose[1], sz + pose[2]], 1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def triangle_setup(P, faces):
    """(N, A, Bv [T, 3], c [T]) of the posed vertices P."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    v0, v1, v2 = P[f[:, 0]], P[f[:, 1]], P[f[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    N, A, Bv = _cross(e1, e2), _cross(e2, v0), _cross(v0, e1)
    c = (v0[:, 0] * N[:, 0] + v0[:, 1] * N[:, 1]) + v0[:, 2] * N[:, 2]
    return N, A, Bv, c


def posed_centroid(P, faces):
    """trimesh's mesh.centroid of the posed mesh."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f):
        tri = P[f]
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        if area.sum() > 0:
            return (tri.mean(1) * area[:, None]).sum(0) / area.sum()
    return P.mean(0) if len(P) else np.zeros(3)


def window_columns(first, count):
    """Columns of a window in window order (it may wrap 4499 -> 0)."""
    return (first + np.arange(count)) % HRES


def window(P, faces, margin=1e-6):
    """(first column, columns) of the azimuth window: the complement of the largest gap no triangle covers; (0, 4500) when a triangle's xy
    projection holds the z axis or nothing is uncovered; (0, 0) without a triangle of non-zero area.  margin: columns added to both
    ends of every triangle's interval."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(f):
        return 0, 0
    N = triangle_setup(P, f)[0]
    f = f[np.any(N != 0, 1)]
    if not len(f):
        return 0, 0
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
    col = lambda p: (np.arctan2(p[:, 0], p[:, 1]) * 57.29577951308232 + 180.0) * (HRES / 360.0)
    c0 = col(a)
    d1, d2 = col(b) - c0, col(d) - c0
    d1 -= HRES * np.rint(d1 / HRES); d2 -= HRES * np.rint(d2 / HRES)
    lo, hi = c0 + np.minimum(0.0, np.minimum(d1, d2)), c0 + np.maximum(0.0, np.maximum(d1, d2))
    full |= hi - lo >= HRES / 2 - 1.0
    if full.any():
        return 0, HRES
    cov = np.zeros(HRES, bool)
    for ca, cb in zip(np.floor(lo - margin).astype(np.int64), np.ceil(hi + margin).astype(np.int64)):
        cov[np.arange(ca, cb + 1) % HRES] = True
    if cov.all():
        return 0, HRES
    # the largest circular run of uncovered columns
    start = int(np.flatnonzero(cov)[0])
    rolled = np.roll(cov, -start)          # rolled[0] is covered
    best_len, best_start, run = 0, 0, 0
    for i in range(1, HRES + 1):
        if i < HRES and not rolled[i]:
            run += 1
        else:
            if run > best_len:
                best_len, best_start = run, i - run
            run = 0
    first = (start + best_start + best_len) % HRES
    return first, HRES - best_len


def cast(P, faces, columns, tables=None, chunk=48):
    """All 64 rows of the given columns against the posed triangles.  Returns dict(t, triangle [64, n] of the plain cast (inf / -1 = miss),
    t_dilated, t_eroded, undecided [64, n] bool)."""
    dx, dy, dz = sensor_tables() if tables is None else tables
    columns = np.asarray(columns, np.int64)
    n = len(columns)
    out = {k: np.full((VRES, n), np.inf) for k in ("t", "t_dilated", "t_eroded")}
    out["triangle"] = np.full((VRES, n), -1, np.int64)
    N, A, Bv, c = triangle_setup(P, faces)
    if len(c):
        nn = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            for k0 in range(0, n, chunk):
                cols = columns[k0:k0 + chunk]
                X, Y, Z = dx[cols][None, :, None], dy[cols][None, :, None], dz[:, None, None]
                dot = lambda V: (X * V[:, 0] + Y * V[:, 1]) + Z * V[:, 2]
                den, un, vn = dot(N), dot(A), dot(Bv)
                u, v, t = un / den, vn / den, c / den
                dn = np.abs(den) / (np.sqrt((X * X + Y * Y) + Z * Z) * nn)
                w = 1.0 - u - v
                hits = {"t": (den != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0),
                        "t_dilated": (dn > 0) & (u >= -EPS) & (v >= -EPS) & (w >= -EPS) & (t > 0),
                        "t_eroded": (dn > EPS) & (u >= EPS) & (v >= EPS) & (w >= EPS) & (t > 0)}
                for key, hit in hits.items():
                    tt = np.where(hit, t, np.inf)
                    out[key][:, k0:k0 + len(cols)] = tt.min(2)
                    if key == "t":
                        best = tt.argmin(2)                      # the first index of the smallest t
                        out["triangle"][:, k0:k0 + len(cols)] = np.where(np.isfinite(tt.min(2)), best, -1)
    td, te = out["t_dilated"], out["t_eroded"]
    both = np.isfinite(td) & np.isfinite(te)
    gap = np.abs(np.where(both, td, 0.0) - np.where(both, te, 0.0))
    out["undecided"] = (np.isfinite(td) != np.isfinite(te)) | (both & (gap > T_TOL))
    return out


def reintersect(P, faces, triangle, columns, tables=None):
    """t and the smallest barycentric (u, v, 1 - u - v) of ray (row, columns[k]) against triangle[row, k] (nan where triangle < 0)."""
    dx, dy, dz = sensor_tables() if tables is None else tables
    N, A, Bv, c = triangle_setup(P, faces)
    tri = np.asarray(triangle)
    ok = tri >= 0
    i = np.where(ok, tri, 0)
    X, Y, Z = dx[np.asarray(columns)][None, :], dy[np.asarray(columns)][None, :], dz[:, None]
    if not len(c):
        return np.full(tri.shape, np.nan), np.full(tri.shape, np.nan)
    dot = lambda V: (X * V[i, 0] + Y * V[i, 1]) + Z * V[i, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = dot(N)
        u, v, t = dot(A) / den, dot(Bv) / den, c[i] / den
    return np.where(ok, t, np.nan), np.where(ok, np.minimum(np.minimum(u, v), 1.0 - u - v), np.nan)


def normals(seed, scene_id, cloud, rays):
    """z [n, 3] float32 of the given ray indices: oracle/dataset_ref.py's stream with the key (seed, scene id, 2 ray + cloud)."""
    rays = np.asarray(rays, np.uint64)
    with np.errstate(over="ignore"):
        key = mix64(np.uint64(seed) ^ (np.uint64(scene_id) * np.uint64(0x9E3779B97F4A7C15)) ^
                    ((np.uint64(2) * rays + np.uint64(cloud)) * np.uint64(0xD1B54A32D192ED03)))
        k2 = mix64(key + np.uint64(0x632BE59BD9B4E019)); k3 = mix64(key + np.uint64(0xC6BC279692B5C323))
    f = np.float32(1.0 / 16777216.0)
    u0 = ((k2 >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * f
    u1 = ((k2 >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * f
    u2 = ((k3 >> np.uint64(40)).astype(np.float32) + np.float32(0.5)) * f
    u3 = ((k3 >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * f
    r0 = np.sqrt(np.float32(-2.0) * np.log(u0)); r1 = np.sqrt(np.float32(-2.0) * np.log(u2))
    tp = np.float32(6.28318530718)
    return np.stack([r0 * np.cos(tp * u1), r0 * np.sin(tp * u1), r1 * np.cos(tp * u3)], 1).astype(np.float32)


def strength(P, faces, sigma):
    return max(0.005, sigma * float(np.linalg.norm(posed_centroid(P, faces))) / 80.)


def cloud(vertices, faces, scale, pose, win=None, tables=None, seed=0, scene_id=0, which=0, sigma=0.0, clip=0.05):
    """One cloud: dict(points float32 [n, 3] in ascending ray index, rays [n] their ray indices, undecided [m] ray indices, window, cast).
    win: the (first, count) window to cast (None: this file's own)."""
    tables = sensor_tables() if tables is None else tables
    P = pose_vertices(vertices, scale, pose)
    first, count = window(P, faces) if win is None else win
    cols = window_columns(first, count)
    res = cast(P, faces, cols, tables)
    ray = np.arange(VRES)[:, None] * HRES + cols[None, :]
    hit = np.isfinite(res["t"])
    order = np.argsort(ray[hit], kind="stable")
    rays = ray[hit][order]
    t = res["t"][hit][order]
    loc = np.stack([t * tables[0][rays % HRES], t * tables[1][rays % HRES], t * tables[2][rays // HRES]], 1)
    pts = loc.astype(np.float32)
    if sigma > 0:
        s = np.float32(strength(P, faces, sigma))
        pts = pts + np.clip(s * normals(seed, scene_id, which, rays), -np.float32(clip), np.float32(clip))
    return dict(points=pts, rays=rays, locations=loc, undecided=np.sort(ray[res["undecided"]]), window=(first, count), cast=res, posed=P)
