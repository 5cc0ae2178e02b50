"""CPU restatement of Open3D's point-to-point ICP with the FULL-rotation estimate (with_constraint=False, icp.py:69-78 as called by the
ICP baseline evaluation, icp.py:150-213), for the tests of alignnet_icp_register* (csrc/alignnet_icp.hip, icp_kernel<true>).

TEST INFRASTRUCTURE ONLY.  The loop, the correspondence step and the stopping rule are oracle/icp_ref.py's (reused from there); the estimate
is Eigen::umeyama(src, dst, with_scaling=false) over the inlier correspondences, restated from its published algorithm:
    means p_bar, q_bar;  Sigma = (1/n) sum (q - q_bar)(p - p_bar)^T = U S V^T (singular values descending);
    D = diag(1, 1, sign(det U det V));  R = U D V^T;  t = q_bar - R p_bar;  T <- [R t] T.
"""
import numpy as np

from oracle.icp_ref import _evaluate, _estimate_z


def estimate_full(p, q):
    if len(p) == 0:
        return np.eye(4)
    mp, mq = p.mean(0), q.mean(0)
    S = (q - mq).T @ (p - mp) / len(p)
    U, _, Vt = np.linalg.svd(S)
    D = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    out = np.eye(4)
    out[:3, :3] = U @ D @ Vt
    out[:3, 3] = mq - out[:3, :3] @ mp
    return out


def icp_p2point(src, dst, init=None, radius=0.1, its=30, with_constraint=False):
    """Returns (T [4,4] float64, fitness, inlier_rmse, iterations run); with_constraint=True is oracle/icp_ref.py's icp_p2point_z."""
    estimate = _estimate_z if with_constraint else estimate_full
    src, dst = np.asarray(src, np.float64)[:, :3], np.asarray(dst, np.float64)[:, :3]
    T = np.eye(4) if init is None else np.array(init, np.float64)
    if len(src) == 0 or len(dst) == 0:
        return T, 0.0, 0.0, 0
    p, q, fit, rmse = _evaluate(src, dst, T, radius)
    k = 0
    for k in range(1, its + 1):
        T = estimate(p, q) @ T
        p, q, nfit, nrmse = _evaluate(src, dst, T, radius)
        done = abs(nfit - fit) < 1e-6 and abs(nrmse - rmse) < 1e-6
        fit, rmse = nfit, nrmse
        if done:
            break
    return T, fit, rmse, k


def centroid_init(src, dst):
    """icp.py:62-66 get_centroid_init: identity rotation, translation = mean(dst) - mean(src) in float64."""
    T = np.eye(4)
    T[:3, 3] = np.asarray(dst, np.float64)[:, :3].mean(0) - np.asarray(src, np.float64)[:, :3].mean(0)
    return T


def rot3(rx, ry, rz):
    """Rz @ Ry @ Rx."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pairs_3d(n_pairs, seed, n2_range=(300, 900), offset=0.0, tilt=0.1):
    """Target clouds and 70 % subsets of them moved by a 3-D motion (tilts up to `tilt` rad about every axis, translation up to 6 cm);
    every third source gets 4 mm of noise.  Returns (sources, targets, inits, truths): inits are the truth disturbed by a small 3-D motion."""
    rng = np.random.default_rng(seed)
    src, dst, inits, truth = [], [], [], []
    for k in range(n_pairs):
        n2 = int(rng.integers(*n2_range))
        q = (rng.uniform(-1, 1, (n2, 3)) * [2.2, 0.9, 0.7] + rng.uniform(-15, 15, 3) + offset).astype(np.float32)
        R, t = rot3(*rng.uniform(-tilt, tilt, 3)), rng.uniform(-0.06, 0.06, 3)
        keep = rng.permutation(n2)[: int(n2 * 0.7)]
        qc = q.astype(np.float64).mean(0)
        p = ((q[keep].astype(np.float64) - qc - t) @ R + qc).astype(np.float32)       # q - qc = R (p - qc) + t
        if k % 3 == 1:
            p = p + rng.normal(0, 0.004, p.shape).astype(np.float32)
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = qc + t - R @ qc
        E = np.eye(4); E[:3, :3] = rot3(*rng.normal(0, 0.01, 3)); E[:3, 3] = qc + rng.normal(0, 0.01, 3) - E[:3, :3] @ qc
        src.append(p); dst.append(q); truth.append(T); inits.append(E @ T)
    return src, dst, inits, truth
