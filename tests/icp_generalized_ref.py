"""fp64 restatement of GENERALIZED (plane-to-plane) ICP, the definition of alignnet_icp_generalized_register* (csrc/alignnet_icp.hip:
icp_surface_kernel<true, .> and the normals kernels run on both clouds) -- tests/test_icp_generalized_cpu.py and tests/test_icp_generalized_gpu.py.
TEST INFRASTRUCTURE ONLY; NumPy fp64 throughout.  Normals, evaluation, transform, solve and the input builders are tests/icp_plane_ref.py's.

Method: Segal, Haehnel, Thrun, "Generalized-ICP" (2009), with the surface covariances of Open3D's registration_generalized_icp (epsilon = 1e-3).
Nothing in the reference pins the arithmetic; this file does.

Normals, once per call, of BOTH clouds, each on its own by the rule of icp_plane_ref.normals (all points of the same cloud within normal_radius, the
point itself included; K < 3: (0, 0, 1); else the smallest eigenvector with n_z >= 0).  The source's are taken in the source's own frame.

Covariances are never stored: a point with unit normal n has C = I - (1 - EPS) n n^T (EPS along the normal, 1 across it).

Loop: icp_plane_ref's -- evaluate, stop test, estimate, T <- U T; correspondence = nearest target within `radius` by point distance, lowest index on
ties; fitness and rmse of point distances; p and the squared distance by icp_plane_ref.transform / evaluate (no fused operation).

Estimate over the inliers (p, q, n_q, n_p), R = the rotation of the current T, K = 1 - EPS, every expression evaluated as written, left to right
inside the parentheses shown, without fused operations:
  m_r   = (R_r0 n_px + R_r1 n_py) + R_r2 n_pz
  A_ii  = 2 - K (n_qi n_qi + m_i m_i),  A_ij = -(K (n_qi n_qj + m_i m_j))                    (= C_q + R C_p R^T, symmetric, eigenvalues in [2 EPS, 2])
  cofactors c00 = A11 A22 - A12 A12, c01 = A02 A12 - A01 A22, c02 = A01 A12 - A02 A11, c11 = A00 A22 - A02 A02, c12 = A01 A02 - A00 A12,
            c22 = A00 A11 - A01 A01;  det = (A00 c00 + A01 c01) + A02 c02;  M_ij = c_ij / det
  d = p - q,  a = p - c (c = the pair's first target point)
  J = [e_x x a, e_y x a, e_z x a, I] = columns (0, -a_z, a_y), (a_z, 0, -a_x), (-a_y, a_x, 0), e_x, e_y, e_z (full) or [e_z x a, I] (z-constrained)
  W = M J:    W_rk = (M_r0 J_0k + M_r1 J_1k) + M_r2 J_2k
  (J^T M J)_kl = (J_0k W_0l + J_1k W_1l) + J_2k W_2l   for k <= l, row by row
  w = M d:    w_r = (M_r0 d_x + M_r1 d_y) + M_r2 d_z;   (J^T M d)_k = (J_0k w_0 + J_1k w_1) + J_2k w_2
The zeros and ones of J are multiplied as any other entry (x * 0 = 0, x + 0 = x and x * 1 = x are exact, so leaving them out changes no bit as
long as no entry is infinite or NaN).
Sums, the slots of point-to-plane: count, sum |d|^2 (the evaluation's squared distances), the upper triangle of sum J^T M J row by row (10 / 21),
sum J^T M d (4 / 6).  Solve (J^T M J) x = -J^T M d and the update U: icp_plane_ref.solve, unchanged.

On the device: p, the squared distance, m, A, the cofactors, det, M, W, w and every term of the sums are evaluated in this order without contraction
and are EXACT TO THE BIT given the same normals and correspondence.  Held to a tolerance: the normals (1e-8: another eigen-solver), the sums
(another order of summation: every sum within 64 n u of the sum of its terms' magnitudes, n = the inliers, u = 2^-53 -- the worst-case bound of an
n-term sum in any order is (n - 1) u; 64 leaves room for the term-level rounding that the magnitudes themselves carry), the update (1e-9 from the
device's sums) and whole runs (1e-9, the bars of icp_plane_ref)."""
import numpy as np
from scipy.spatial import cKDTree

from tests import icp_plane_ref as P

EPS = 1e-3                         # Open3D's epsilon: the covariance along the normal
KAPPA = 1.0 - EPS
U64 = P.U64
TRI = P.TRI


def nsums(full):
    return 29 if full else 16


# ---- per-correspondence pieces ---------------------------------------------------------------------------------------------------------------
def rotate(R, n):
    """m = R n per row, unfused."""
    R, n = np.asarray(R, np.float64), np.asarray(n, np.float64).reshape(-1, 3)
    return np.stack([(R[r, 0] * n[:, 0] + R[r, 1] * n[:, 1]) + R[r, 2] * n[:, 2] for r in range(3)], 1)


def cov_sum(nq, m):
    """A [n, 3, 3] = C_q + R C_p R^T from the unit normals nq and m = R n_p."""
    nq, m = np.asarray(nq, np.float64).reshape(-1, 3), np.asarray(m, np.float64).reshape(-1, 3)
    A = np.zeros((len(nq), 3, 3))
    for i in range(3):
        for j in range(i, 3):
            s = KAPPA * (nq[:, i] * nq[:, j] + m[:, i] * m[:, j])
            A[:, i, j] = A[:, j, i] = (2.0 - s) if i == j else -s
    return A


def inverse3(A):
    """Closed-form inverse of symmetric 3x3 matrices [n, 3, 3] (cofactors / determinant)."""
    A = np.asarray(A, np.float64).reshape(-1, 3, 3)
    a00, a01, a02, a11, a12, a22 = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    M = np.zeros_like(A)
    M[:, 0, 0] = c00 / det
    M[:, 0, 1] = M[:, 1, 0] = c01 / det
    M[:, 0, 2] = M[:, 2, 0] = c02 / det
    M[:, 1, 1] = c11 / det
    M[:, 1, 2] = M[:, 2, 1] = c12 / det
    M[:, 2, 2] = c22 / det
    return M


def jacobian(p, c, full):
    """J [n, 3, N]: columns e_k x a (k = x, y, z when full, z alone otherwise), then the identity."""
    a = np.asarray(p, np.float64).reshape(-1, 3) - np.asarray(c, np.float64)
    n = len(a)
    z, o = np.zeros(n), np.ones(n)
    cols = []
    if full:
        cols += [np.stack([z, -a[:, 2], a[:, 1]], 1), np.stack([a[:, 2], z, -a[:, 0]], 1)]
    cols += [np.stack([-a[:, 1], a[:, 0], z], 1), np.stack([o, z, z], 1), np.stack([z, o, z], 1), np.stack([z, z, o], 1)]
    return np.stack(cols, 2)


def weights(nq, n_p, T):
    """M [n, 3, 3] of the correspondences under the current transform."""
    return inverse3(cov_sum(nq, rotate(np.asarray(T, np.float64)[:3, :3], n_p)))


def terms(p, q, M, best, c, full):
    """The per-correspondence terms of the 16 / 29 sums, as columns [n, nsums]."""
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    J = jacobian(p, c, full)
    N = J.shape[2]
    d = p - q
    W = np.stack([np.stack([(M[:, r, 0] * J[:, 0, k] + M[:, r, 1] * J[:, 1, k]) + M[:, r, 2] * J[:, 2, k] for k in range(N)], 1) for r in range(3)], 1)
    w = np.stack([(M[:, r, 0] * d[:, 0] + M[:, r, 1] * d[:, 1]) + M[:, r, 2] * d[:, 2] for r in range(3)], 1)
    cols = [np.ones(len(p)), np.asarray(best, np.float64)]
    cols += [(J[:, 0, k] * W[:, 0, l] + J[:, 1, k] * W[:, 1, l]) + J[:, 2, k] * W[:, 2, l] for k, l in TRI[full]]
    cols += [(J[:, 0, k] * w[:, 0] + J[:, 1, k] * w[:, 1]) + J[:, 2, k] * w[:, 2] for k in range(N)]
    return np.stack(cols, 1) if len(p) else np.zeros((0, nsums(full)))


def sums(p, q, nq, n_p, T, best, c, full):
    """(sums [29], magnitudes [29], n): as icp_plane_ref.sums."""
    t = terms(p, q, weights(nq, n_p, T), best, c, full)
    s, mag = np.zeros(29), np.zeros(29)
    s[: t.shape[1]], mag[: t.shape[1]] = t.sum(0), np.abs(t).sum(0)
    return s, mag, len(t)


def objective(p, q, M):
    """sum d^T M d (M held fixed): what one Gauss-Newton step of the estimate minimises to first order."""
    d = np.asarray(p, np.float64) - np.asarray(q, np.float64)
    return float(np.einsum("ni,nij,nj->", d, M, d))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
# icp_plane_ref.BATCH_SIZES with its single planes of 1, 2 and 3 targets (1, 1 and 2 source points) replaced by planes of 8, 12 and 20 (5, 8 and 13
# source points): one or two correspondences leave a rotation exactly undetermined (a pivot of rounding noise), which is neither of the two classes
# the whole-run comparison rests on -- no correspondence, or a scaled condition number <= 1e4 (tests/test_icp_generalized_cpu.py checks every
# estimate of these pairs).  Sources of 1, 2 and 3 points go through the debug hook instead (tests/test_icp_generalized_gpu.py).
BATCH_SIZES = (700, 0, 63, 8, 256, 12, 1025, 20, 300, 5, 64, 6000, 65, 255, 1500, 257, 1023, 3000, 1024, 40, 450, 2100, 130, 4267)


def batch_pairs(n_pairs=70, seed=300):
    """icp_plane_ref.batch_pairs on BATCH_SIZES above: 70 heterogeneous pairs, targets of 0 to 6,000 points; box corners from 63 points on, every
    third with a 3-D motion, single planes below; pair 1 has an empty target, pair 4 an empty source.  Returns (sources, targets, inits)."""
    srcs, dsts, inits = [], [], []
    for k in range(n_pairs):
        base = BATCH_SIZES[k % len(BATCH_SIZES)]
        n2 = base + (k // len(BATCH_SIZES)) * 7 * (base > 63)
        if n2 < 63:
            src, dst = P.plane_pair(n2, seed + k) if n2 else (np.zeros((5, 3), np.float32), np.zeros((0, 3), np.float32))
            init = np.eye(4)
        else:
            src, dst, init, _ = P.corner_pair(n2, seed + k, offset=float(7 * (k % 5)), constrained=k % 3 != 0, side=max(0.6, 1.5 * np.sqrt(n2 / 600.0)))
        if k == 4:
            src = src[:0]
        srcs.append(src); dsts.append(dst); inits.append(init)
    return srcs, dsts, inits


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
def icp_generalized(src, dst, init, radius=0.1, normal_radius=0.3, its=30, constrained=True, nrm_dst=None, nrm_src=None, info=None):
    """Returns (T [4, 4], fitness, rmse, iterations, undecided) as icp_plane_ref.icp_plane; undecided counts, per evaluation, the source points within
    the margins of a correspondence decision and the inliers whose target or source normal is within the margins of its own decisions."""
    src, dst = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(dst, np.float64).reshape(-1, 3)
    T = np.array(init, np.float64).reshape(4, 4)
    full = not constrained
    if info is not None:
        info.update(conds=[], determined=[], evaluations=0)
    if len(src) == 0 or len(dst) == 0:
        return T, 0.0, 0.0, 0, 0
    nrm_dst = P.normals(dst, normal_radius) if nrm_dst is None else nrm_dst
    nrm_src = P.normals(src, normal_radius) if nrm_src is None else nrm_src
    und_q, und_p = P.normals_undecided(nrm_dst), P.normals_undecided(nrm_src)
    c = dst[0]
    und = 0
    tree = cKDTree(dst)

    def step(T):
        e = P.evaluate(src, dst, T, radius, tree)
        i = e["inlier"]
        j = e["index"][i]
        u = int(e["undecided"].sum()) + int(und_q[j].sum()) + int(und_p[i].sum())
        return e, sums(e["p"][i], dst[j], nrm_dst["normals"][j], nrm_src["normals"][i], T, e["best"][i], c, full)[0], u

    e, s, u = step(T)
    und += u
    fit, rmse = e["fitness"], e["rmse"]
    k = 0
    for k in range(1, its + 1):
        si = {}
        U, ok = P.solve(s, c, full, si)
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
