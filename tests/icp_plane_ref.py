"""fp64 restatement of POINT-TO-PLANE ICP, the definition of alignnet_icp_plane_register* (csrc/alignnet_icp.hip: icp_plane_normals_kernel,
icp_surface_kernel<false, .>) -- tests/test_icp_plane_cpu.py and tests/test_icp_plane_gpu.py.  TEST INFRASTRUCTURE ONLY; NumPy fp64 throughout (scipy's cKDTree
only proposes neighbour candidates, every decision is taken on distances computed here).

The reference names the method and leaves it `assert False` (icp.py:81-82), so nothing pins the arithmetic but this file.

Target normals, once per call, for every target point q_i: the neighbours are all targets with ((dx^2 + dy^2) + dz^2) <= fl(normal_radius^2) in fp64
(dx = q_j - q_i; the point itself included; no cap on their number).  K < 3: (0, 0, 1).  Else the covariance S2 / K - m m^T of the differences
(m = S1 / K: one pass, about the query point), its unit eigenvector of the smallest eigenvalue, flipped so that n_z >= 0.

Loop: oracle/icp_ref.py's -- evaluate, stop test (|d fitness| < 1e-6 and |d rmse| < 1e-6), estimate, T <- U T; the correspondence of a source point
is the nearest target within `radius` by point distance, lowest index on ties; fitness and rmse are of point distances.  The transformed point is
p_x = ((T00 s_x + T01 s_y) + T02 s_z) + T03 (no fused operation), the squared distance ((dx^2 + dy^2) + dz^2) with dx = p_x - q_x.

Estimate over the inlier correspondences (p, q, n), c = the pair's first target point (the kernels' pivot): r = ((dx n_x + dy n_y) + dz n_z),
a = p - c; full rotation J = [a x n, n] (6 columns, x = (alpha, beta, gamma, t)), z-constrained J = [(a x n)_z, n] (4 columns, x = (gamma, t));
J^T J x = -J^T r solved by Cholesky without pivoting on the diagonally scaled matrix D A D, D = diag(A)^-1/2; U = Tr(c) [Rz(gamma) Ry(beta) Rx(alpha) | t]
Tr(-c).  No correspondence, a diagonal entry <= 0 or a pivot <= PIVOT: no update is determined, U = I.  (About c the linear system has the minimiser
of Open3D's about the origin; the rotation is then applied about c, which differs at second order in the angle: this file is the definition.)"""
import numpy as np
from scipy.spatial import cKDTree

from tests.icp_full_ref import rot3

PIVOT = 1e-10                      # on the scaled matrix (unit diagonal)
UNDECIDED, UNDECIDED_GAP, SKIP_CAP, REF_CAP = 1e-9, 1e-6, 1e-3, 1e-4     # the constants of tests/global_reg_ref.py; REF_CAP: the restatement alone
U64 = 2.0 ** -53
TRI = {True: [(i, j) for i in range(6) for j in range(i, 6)], False: [(i, j) for i in range(4) for j in range(i, 4)]}


def nsums(full):
    return 29 if full else 16


# ---- normals -----------------------------------------------------------------------------------------------------------------------------
def normals(dst, normal_radius):
    """dict(normals [n2, 3], count [n2], nbr_margin [n2] = min |d^2 - r^2| / r^2 over the candidates, gap [n2] = (l1 - l0) / l2, nz [n2] = |n_z|;
    gap and nz are inf where K < 3: nothing to decide there but the count)."""
    q = np.asarray(dst, np.float64).reshape(-1, 3)
    m = len(q)
    out = dict(normals=np.tile([0.0, 0.0, 1.0], (m, 1)), count=np.zeros(m, np.int64), nbr_margin=np.full(m, np.inf), gap=np.full(m, np.inf),
               nz=np.full(m, np.inf))
    if m == 0:
        return out
    r2 = normal_radius * normal_radius
    lists = cKDTree(q).query_ball_point(q, normal_radius * (1 + 1e-6) + 1e-12, return_sorted=True)
    I = np.repeat(np.arange(m), [len(l) for l in lists])
    J = np.concatenate([np.asarray(l, np.int64) for l in lists])
    d = q[J] - q[I]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    np.minimum.at(out["nbr_margin"], I, np.abs(d2 - r2) / r2)
    keep = d2 <= r2
    I, d = I[keep], d[keep]
    K = np.bincount(I, minlength=m)
    out["count"] = K
    S1 = np.stack([np.bincount(I, weights=d[:, k], minlength=m) for k in range(3)], 1)
    S2 = np.stack([np.bincount(I, weights=d[:, a] * d[:, b], minlength=m) for a in range(3) for b in range(3)], 1).reshape(m, 3, 3)
    ok = K >= 3
    Kf = np.maximum(K, 1)[:, None].astype(np.float64)
    mean = S1 / Kf
    cov = S2 / Kf[:, :, None] - mean[:, :, None] * mean[:, None, :]
    w, v = np.linalg.eigh(cov[ok])
    n = v[:, :, 0]
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    n[n[:, 2] < 0] *= -1.0
    out["normals"][ok] = n
    out["gap"][ok] = (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-300)
    out["nz"][ok] = np.abs(n[:, 2])
    return out


def normals_undecided(nr):
    return (nr["nbr_margin"] < UNDECIDED) | (nr["gap"] < UNDECIDED_GAP) | (nr["nz"] < UNDECIDED)


# ---- one evaluation ------------------------------------------------------------------------------------------------------------------------
def transform(src, T):
    s = np.asarray(src, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64)
    return np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], 1)


def evaluate(src, dst, T, radius, tree=None, k=4):
    """dict(p [n1, 3], index [n1] (lowest index of the nearest target), best [n1] its squared distance, inlier [n1], fitness, rmse,
    undecided [n1]: the relative gap to the second-best distance or the margin to radius^2 is under UNDECIDED).  The tree proposes the k nearest
    targets; their distances are computed here and the smallest (distance, index) is taken (more than k targets in an exact tie: undecided)."""
    p, q = transform(src, T), np.asarray(dst, np.float64).reshape(-1, 3)
    n1, r2 = len(p), radius * radius
    k = min(k, len(q))
    tree = cKDTree(q) if tree is None else tree
    _, cand = tree.query(p, k=k)
    cand = np.asarray(cand, np.int64).reshape(n1, k)
    d = p[:, None, :] - q[cand]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    order = np.lexsort((cand, d2), axis=1)
    ar = np.arange(n1)
    index, best = cand[ar, order[:, 0]], d2[ar, order[:, 0]]
    second = d2[ar, order[:, 1]] if k > 1 else np.full(n1, np.inf)
    inlier = best <= r2
    tie = (second - best) <= UNDECIDED * np.maximum(second, 1e-300)
    tie &= np.isfinite(second) & (best <= r2 * (1 + UNDECIDED))   # (a tie beyond the radius decides nothing)
    edge = np.abs(best - r2) <= UNDECIDED * r2
    n = int(inlier.sum())
    return dict(p=p, index=index, best=best, inlier=inlier, fitness=n / float(n1) if n1 else 0.0,
                rmse=float(np.sqrt(best[inlier].sum() / n)) if n else 0.0, undecided=tie | edge)


def residuals(p, q, n):
    d = p - q
    return (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]


# ---- the estimate ----------------------------------------------------------------------------------------------------------------------------
def jacobian(p, n, c, full):
    a = p - c
    ax, ay, az, nx, ny, nz = a[:, 0], a[:, 1], a[:, 2], n[:, 0], n[:, 1], n[:, 2]
    if full:
        return np.stack([ay * nz - az * ny, az * nx - ax * nz, ax * ny - ay * nx, nx, ny, nz], 1)
    return np.stack([ax * ny - ay * nx, nx, ny, nz], 1)


def sums(p, q, n, best, c, full):
    """(sums [29], magnitudes [29], terms): count, sum d^2, upper triangle of J^T J row by row, J^T r (16 entries used when not full);
    magnitudes = sum |term| of every entry: an n-term fp64 sum in any order lies within about n u of it times the entry's magnitude."""
    J, r = jacobian(p, n, c, full), residuals(p, q, n)
    cols = [np.ones(len(p)), best] + [J[:, i] * J[:, j] for i, j in TRI[full]] + [J[:, i] * r for i in range(J.shape[1])]
    s, mag = np.zeros(29), np.zeros(29)
    for k, col in enumerate(cols):
        s[k], mag[k] = col.sum(), np.abs(col).sum()
    return s, mag, len(p)


def solve(s, c, full, info=None):
    """The update U [4, 4] of the sums `s`, and whether one was determined.  info: dict that receives cond (2-norm condition number of the
    scaled matrix; inf when undetermined) and x."""
    N = 6 if full else 4
    U = np.eye(4)
    if info is not None:
        info["cond"], info["x"] = np.inf, np.zeros(N)
    if not s[0] > 0:
        return U, False
    A = np.zeros((N, N))
    for k, (i, j) in enumerate(TRI[full]):
        A[i, j] = A[j, i] = s[2 + k]
    g = s[2 + len(TRI[full]): 2 + len(TRI[full]) + N]
    if not np.all(np.diag(A) > 0):
        return U, False
    sc = 1.0 / np.sqrt(np.diag(A))
    As = A * sc[:, None] * sc[None, :]
    L = np.zeros((N, N))
    for k in range(N):
        d = As[k, k] - (L[k, :k] * L[k, :k]).sum()
        if not d > PIVOT:
            return U, False
        L[k, k] = np.sqrt(d)
        for i in range(k + 1, N):
            L[i, k] = (As[i, k] - (L[i, :k] * L[k, :k]).sum()) / L[k, k]
    y = np.zeros(N)
    for i in range(N):
        y[i] = (-(sc[i] * g[i]) - (L[i, :i] * y[:i]).sum()) / L[i, i]
    for i in range(N - 1, -1, -1):
        y[i] = (y[i] - (L[i + 1:, i] * y[i + 1:]).sum()) / L[i, i]
    x = y * sc
    if info is not None:
        info["cond"], info["x"] = float(np.linalg.cond(As)), x
    R = rot3(x[0], x[1], x[2]) if full else rot3(0.0, 0.0, x[0])
    t = x[3:] if full else x[1:]
    c = np.asarray(c, np.float64)
    U[:3, :3] = R
    U[:3, 3] = (c + t) - R @ c
    return U, True


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
def icp_plane(src, dst, init, radius=0.1, normal_radius=0.3, its=30, constrained=True, nrm=None, info=None):
    """Returns (T [4, 4], fitness, rmse, iterations, undecided): undecided = entries (normals of the target + source points over all evaluations)
    within the margins of a decision -- a device run may then differ.  nrm: normals() of the target if already computed.
    info: dict that receives conds (one per estimate), determined (one bool per estimate), evaluations."""
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    T = np.array(init, np.float64).reshape(4, 4)
    full = not constrained
    if info is not None:
        info.update(conds=[], determined=[], evaluations=0)
    if len(src) == 0 or len(dst) == 0:
        return T, 0.0, 0.0, 0, 0
    nrm = normals(dst, normal_radius) if nrm is None else nrm
    und_n = normals_undecided(nrm)
    c = dst[0]
    und = 0
    tree = cKDTree(dst)

    def step(T):
        e = evaluate(src, dst, T, radius, tree)
        i = e["inlier"]
        j = e["index"][i]
        u = int(e["undecided"].sum()) + int(und_n[j].sum())
        return e, sums(e["p"][i], dst[j], nrm["normals"][j], e["best"][i], c, full)[0], u

    e, s, u = step(T)
    und += u
    fit, rmse = e["fitness"], e["rmse"]
    k = 0
    for k in range(1, its + 1):
        si = {}
        U, ok = solve(s, c, full, si)
        if info is not None:
            info["conds"].append(si["cond"]); info["determined"].append(ok)
        if ok:
            T = U @ T
        e, s, u = step(T)
        und += u
        done = abs(e["fitness"] - fit) < 1e-6 and abs(e["rmse"] - rmse) < 1e-6
        fit, rmse = e["fitness"], e["rmse"]
        if done:
            break
    if info is not None:
        info["evaluations"] = k + 1
    return T, fit, rmse, k, und


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def box_corner(n, seed, noise=0.002, offset=0.0, side=1.5):
    """n float32 points on the three faces of a box corner at `offset` (+ a fixed shift), `noise` metres along the face normal."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.0, side, (n, 3))
    axis = rng.integers(0, 3, n)
    q[np.arange(n), axis] = rng.normal(0, noise, n)
    return (q + [3.0, -2.0, 0.5] + offset).astype(np.float32)


def rigid_about(centre, angles, shift):
    T = np.eye(4)
    T[:3, :3] = rot3(*angles)
    T[:3, 3] = np.asarray(centre) + shift - T[:3, :3] @ np.asarray(centre)
    return T


def corner_pair(n2, seed, offset=0.0, constrained=True, noise=0.002, side=1.5):
    """(src, dst, init, truth): the source is a 70 % subset of a noisy box corner moved by the inverse of a small motion (about z only when
    constrained); init = the truth disturbed by 2 degrees and 3 cm."""
    rng = np.random.default_rng(seed + 17)
    dst = box_corner(n2, seed, noise, offset, side)
    keep = rng.permutation(n2)[: int(n2 * 0.7)]
    qc = dst.astype(np.float64).mean(0) if n2 else np.zeros(3)
    ang = rng.uniform(-0.05, 0.05, 3) * ([0, 0, 1] if constrained else [1, 1, 1])
    truth = rigid_about(qc, ang, rng.uniform(-0.05, 0.05, 3))
    inv = np.linalg.inv(truth)
    src = (dst[keep].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3] + rng.normal(0, noise, (len(keep), 3))).astype(np.float32)
    dang = np.deg2rad(2.0) * rng.choice([-1.0, 1.0], 3) * ([0, 0, 1] if constrained else [0.3, 0.3, 1])
    init = rigid_about(qc, dang, rng.uniform(-0.03, 0.03, 3)) @ truth
    return src, dst, init, truth


def plane_pair(n, seed, tilt=(0.0, 0.0)):
    """A single plane (exactly rank-deficient for both estimates): dyadic grid coordinates on z = 0.5, optionally tilted by exact small slopes."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 256, (n, 2)).astype(np.float64) / 128.0
    z = 0.5 + tilt[0] * xy[:, 0] + tilt[1] * xy[:, 1]
    dst = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    src = (dst[: max(n * 2 // 3, 1)].astype(np.float64) + [0.0, 0.0, 0.03]).astype(np.float32)
    return src, dst


def car_pair(dist, seed, sigma=0.05, scale=6.0):
    """Two scans of the built-in car by tests/scene_ref.py (noise ON unless sigma = 0) a small motion apart.  Returns (src, dst, truth)."""
    from tests import scene_cases as C
    from tests import scene_ref as R
    rng = np.random.default_rng(seed)
    v, f = C.car()
    bearing, yaw = rng.uniform(-180, 180), rng.uniform(-np.pi, np.pi)
    p1 = C.polar(dist, bearing, yaw=yaw)
    p2 = C.polar(dist + rng.uniform(-0.3, 0.3), bearing + rng.uniform(-2, 2), yaw=yaw + rng.uniform(-0.2, 0.2))
    tabs = R.sensor_tables()
    c1 = R.cloud(v, f, scale, p1, tables=tabs, seed=seed, scene_id=seed, which=0, sigma=sigma)["points"]
    c2 = R.cloud(v, f, scale, p2, tables=tabs, seed=seed, scene_id=seed, which=1, sigma=sigma)["points"]
    T = np.eye(4)
    T[:3, :3] = rot3(0.0, 0.0, p2[3] - p1[3])
    T[:3, 3] = np.asarray(p2[:3]) - T[:3, :3] @ np.asarray(p1[:3])
    return c1, c2, T


def disturbed(truth, centre, degrees=4.0, shift=0.12, seed=0):
    """The truth turned by `degrees` about z through `centre` and shifted by `shift` metres in a random horizontal direction."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi)
    return rigid_about(centre, (0.0, 0.0, np.deg2rad(degrees) * rng.choice([-1.0, 1.0])), np.array([np.cos(a), np.sin(a), 0.0]) * shift) @ truth


def pose_error(T, truth, centre):
    """(yaw error in degrees, translation error in metres of the point `centre` of the source cloud)."""
    D = T @ np.linalg.inv(truth)
    c = np.append(np.asarray(centre, np.float64), 1.0)
    return abs(np.degrees(np.arctan2(D[1, 0], D[0, 0]))), float(np.linalg.norm((T @ c - truth @ c)[:3]))


BATCH_SIZES = (700, 0, 63, 1, 256, 2, 1025, 3, 300, 5, 64, 6000, 65, 255, 1500, 257, 1023, 3000, 1024, 40, 450, 2100, 130, 4267)


def batch_pairs(n_pairs=70, seed=300):
    """Heterogeneous pairs for one call, sizes 0 to 6,000: targets of 64 points and more are noisy box corners at constant density (about 25
    neighbours within 0.3 m), every third with a 3-D motion; smaller ones are single planes (exactly rank-deficient: no update) -- nothing in
    between; pair 4 has an empty SOURCE.  Returns (sources, targets, inits)."""
    srcs, dsts, inits = [], [], []
    for k in range(n_pairs):
        n2 = BATCH_SIZES[k % len(BATCH_SIZES)] + (k // len(BATCH_SIZES)) * 7 * (BATCH_SIZES[k % len(BATCH_SIZES)] > 63)
        if n2 < 63:
            src, dst = plane_pair(n2, seed + k) if n2 else (np.zeros((5, 3), np.float32), np.zeros((0, 3), np.float32))
            init = np.eye(4)
        else:
            src, dst, init, _ = corner_pair(n2, seed + k, offset=float(7 * (k % 5)), constrained=k % 3 != 0, side=max(0.6, 1.5 * np.sqrt(n2 / 600.0)))
        if k == 4:
            src = src[:0]
        srcs.append(src); dsts.append(dst); inits.append(init)
    return srcs, dsts, inits
