"""NumPy restatement of the Go-ICP baseline (`goicp`, icp.py:146-147: the reference names the method and leaves it `assert False`).

TEST INFRASTRUCTURE ONLY.  The reference has no Go-ICP code to restate, so this text DEFINES what csrc/alignnet_goicp.hip computes
(DESIGN.md 4.7e): a level-synchronous branch-and-bound over yaw and a translation box, z-constrained, on subsampled working sets.

Working sets: S = the source if n1 <= max_source, else its points floor(i n1 / max_source), i < max_source; Q likewise with max_target.
Every decision and sum is fp64 on centred coordinates: c1 = mean(S), cq = mean(Q) (taken as first point + mean of the differences to it,
which is exact for float32 clouds far from the origin), t0 = cq - c1, and
    T(theta, t): x -> Rz(theta)(x - c1) + c1 + t0 + t          theta in [-yaw_half, yaw_half], t_k in [-t_half[k], t_half[k]]
    d_i = min_j |T(s_i) - q_j|,   E = sum_i min(d_i, trunc)^2.
A node is a box with half-widths (delta, a) around its centre; with rho_i the xy-norm of s_i - c1,
    gamma_i = 2 rho_i sin(min(delta, pi) / 2) + |a|_2,   ub = E(centre),   lb = sum_i min(max(d_i(centre) - gamma_i, 0), trunc)^2.
All nodes of a level share their depths: dimension k (theta, x, y, z) has been halved depth[k] times, a node carries the integer
coordinate i_k in [0, 2^depth[k]) and its centre is (2 i_k + 1 - 2^depth[k]) * (half[k] 2^-depth[k]), one rounding.
Search, per level: evaluate the frontier; the lowest ub (lowest frontier index on a tie) replaces the best pose if it is smaller;
keep the nodes with lb < best - eps, eps = mse_thresh |S|; stop CERTIFIED when none is left, RESOLUTION when no dimension's half-width
is above its resolution, LEVELS when max_levels levels have been evaluated, OVERFLOW when survivors x children > max_frontier; else
split every dimension still above its resolution, children in lexicographic (theta, x, y, z) order, survivors in their parents' order.
lower_bound = min(error - eps, min lb of the nodes still open).  Initial bound: `starts` z-constrained point-to-point ICP runs
(oracle/icp_ref.py) on the float32 working sets from yaws 2 pi k / starts about c1 plus t0; a start that ends outside the domain is
discarded, the others' exact E compete (the earliest on a tie; a frontier node must be strictly smaller to replace them)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import icp_ref  # noqa: E402

CERTIFIED, RESOLUTION, OVERFLOW, LEVELS, EMPTY = 0, 1, 2, 3, 4
STATUS_NAMES = ("CERTIFIED", "RESOLUTION", "OVERFLOW", "LEVELS", "EMPTY")
MAX_LEVELS = 24

DEFAULTS = dict(yaw_half=np.pi, t_half=(2.0, 2.0, 0.25), yaw_res=np.pi / 256, t_res=0.02, trunc=0.5, mse_thresh=1e-4, max_source=256,
                max_target=2048, max_frontier=1 << 18, max_levels=MAX_LEVELS, starts=8, start_radius=0.5, start_its=30, fitness_radius=0.10, stage_points=0)


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    p["t_half"] = tuple(float(x) for x in p["t_half"])
    return p


def working_set(pts, cap):
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    n = len(pts)
    if n <= cap:
        return pts
    return pts[(np.arange(cap, dtype=np.int64) * n) // cap]


def mean64(pts32):
    p = np.asarray(pts32, np.float64)
    return p[0] + (p - p[0]).mean(0)


class Problem:
    """The centred working sets of one pair."""

    def __init__(self, source, target, p):
        self.p = p
        self.S32, self.Q32 = working_set(source, p["max_source"]), working_set(target, p["max_target"])
        self.empty = len(self.S32) == 0 or len(self.Q32) == 0
        if self.empty:
            return
        self.c1, self.cq = mean64(self.S32), mean64(self.Q32)
        self.Sc = self.S32.astype(np.float64) - self.c1
        self.Qc = self.Q32.astype(np.float64) - self.cq
        self.rho = np.sqrt(self.Sc[:, 0] ** 2 + self.Sc[:, 1] ** 2)
        self.half = np.array((p["yaw_half"],) + p["t_half"], np.float64)
        self.res = np.array((p["yaw_res"], p["t_res"], p["t_res"], p["t_res"]), np.float64)
        self.eps = p["mse_thresh"] * len(self.Sc)

    def dists(self, theta, t):
        """d_i at the pose: [ns] fp64, by differences (no expansion)."""
        c, s = np.cos(theta), np.sin(theta)
        x = np.stack([c * self.Sc[:, 0] - s * self.Sc[:, 1] + t[0], s * self.Sc[:, 0] + c * self.Sc[:, 1] + t[1], self.Sc[:, 2] + t[2]], 1)
        d2 = ((x[:, None, :] - self.Qc[None, :, :]) ** 2).sum(-1).min(1)
        return np.sqrt(d2)

    def energy(self, theta, t):
        return float((np.minimum(self.dists(theta, t), self.p["trunc"]) ** 2).sum())

    def widths(self, depth):
        return np.ldexp(self.half, -np.asarray(depth, np.int64))

    def centres(self, depth, coords):
        """coords [K, 4] integers -> poses [K, 4] (theta, tx, ty, tz)."""
        coords = np.asarray(coords, np.int64).reshape(-1, 4)
        depth = np.asarray(depth, np.int64)
        return (2 * coords + 1 - (1 << depth)).astype(np.float64) * self.widths(depth)

    def gamma(self, depth):
        w = self.widths(depth)
        return 2.0 * np.sin(min(w[0], np.pi) / 2.0) * self.rho + np.sqrt((w[1:] ** 2).sum())

    def dists_many(self, poses):
        """d_i at K poses: [K, ns]."""
        poses = np.asarray(poses, np.float64).reshape(-1, 4)
        out = np.empty((len(poses), len(self.Sc)))
        step = max(1, min(32, 1500000 // max(1, len(self.Sc) * len(self.Qc))))   # (the [step, ns, nq, 3] differences stay within tens of MB)
        for k0 in range(0, len(poses), step):
            q = poses[k0:k0 + step]
            c, s = np.cos(q[:, 0])[:, None], np.sin(q[:, 0])[:, None]
            x = np.stack([c * self.Sc[:, 0] - s * self.Sc[:, 1] + q[:, 1:2], s * self.Sc[:, 0] + c * self.Sc[:, 1] + q[:, 2:3],
                          self.Sc[:, 2] + q[:, 3:4]], -1)
            out[k0:k0 + step] = np.sqrt(((x[:, :, None, :] - self.Qc[None, None, :, :]) ** 2).sum(-1).min(-1))
        return out

    def energies(self, poses):
        return (np.minimum(self.dists_many(poses), self.p["trunc"]) ** 2).sum(1)

    def bounds(self, depth, coords):
        """(ub [K], lb [K]) of the nodes."""
        d = self.dists_many(self.centres(depth, coords))
        g, tr = self.gamma(depth), self.p["trunc"]
        return (np.minimum(d, tr) ** 2).sum(1), (np.minimum(np.maximum(d - g, 0.0), tr) ** 2).sum(1)

    def transform(self, pose):
        """x -> Rz(theta)(x - c1) + cq + t as a 4x4 about the origin."""
        c, s = np.cos(pose[0]), np.sin(pose[0])
        T = np.eye(4)
        T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
        T[:3, 3] = self.cq + np.asarray(pose[1:]) - T[:3, :3] @ self.c1
        return T

    def pose_of(self, T):
        """The (theta, t) of a z-rotation 4x4 in this problem's parametrisation."""
        th = np.arctan2(T[1, 0], T[0, 0])
        return np.concatenate([[th], T[:3, :3] @ self.c1 + T[:3, 3] - self.cq])

    def start_inits(self):
        n = self.p["starts"]
        return [icp_ref.get_mat_angle(self.cq - self.c1, 2.0 * np.pi * k / n, self.c1) for k in range(n)]


def children(coords, split):
    """coords [m, 4] -> [m 2^|split|, 4]: per survivor, the children in lexicographic (theta, x, y, z) order."""
    out = np.asarray(coords, np.int64).reshape(-1, 1, 4)
    for k in range(4):
        if split[k]:
            lo = out.copy(); lo[..., k] = 2 * out[..., k]
            hi = out.copy(); hi[..., k] = 2 * out[..., k] + 1
            out = np.stack([lo, hi], 2).reshape(out.shape[0], -1, 4)   # dimension k varies slower than the later ones
    return out.reshape(-1, 4)


def search(source, target, p=None, margins=None):
    """One pair.  Returns dict(transform, pose, error, lower_bound, fitness (share of S within fitness_radius at the pose), status, evaluated [MAX_LEVELS], survived [MAX_LEVELS]).
    margins: a list that receives the relative distance of every decision from its threshold (prune tests, best-pose ties)."""
    p = p or params()
    pr = Problem(source, target, p)
    ev, sv = np.zeros(MAX_LEVELS, np.int64), np.zeros(MAX_LEVELS, np.int64)
    if pr.empty:
        return dict(transform=np.eye(4), pose=np.zeros(4), error=0.0, lower_bound=0.0, fitness=0.0, status=EMPTY, evaluated=ev, survived=sv)
    best, pose = np.inf, np.zeros(4)
    for T0 in (pr.start_inits() if p["starts"] > 0 else []):
        T, _, _, _ = icp_ref.icp_p2point_z(pr.S32, pr.Q32, T0, p["start_radius"], p["start_its"])
        q = pr.pose_of(T)
        if np.all(np.abs(q) <= pr.half):
            e = pr.energy(q[0], q[1:])
            if margins is not None and np.isfinite(best):
                margins.append(abs(e - best) / max(abs(best), 1e-300) if e != best else np.inf)   # equal values: the same basin, either pose serves
            if e < best:
                best, pose = e, q
    depth = np.zeros(4, np.int64)
    coords = np.zeros((1, 4), np.int64)
    level = 0
    while True:
        ub, lb = pr.bounds(depth, coords)
        ev[level] = len(coords)
        i = int(np.argmin(ub))
        if margins is not None:
            others = np.delete(ub, i)
            if len(others):
                margins.append((others.min() - ub[i]) / max(abs(ub[i]), 1e-300))
            if np.isfinite(best):
                margins.append(abs(ub[i] - best) / max(abs(best), 1e-300))
        if ub[i] < best:
            best, pose = float(ub[i]), pr.centres(depth, coords[i])[0]
        thr = best - pr.eps
        if margins is not None:
            margins.extend(np.abs(lb - thr) / max(abs(thr), 1e-300))
        keep = lb < thr
        sv[level] = int(keep.sum())
        coords, open_lb = coords[keep], lb[keep]
        split = pr.widths(depth) > pr.res
        if len(coords) == 0:
            status = CERTIFIED
        elif not split.any():
            status = RESOLUTION
        elif level + 1 >= p["max_levels"]:
            status = LEVELS
        elif len(coords) << int(split.sum()) > p["max_frontier"]:
            status = OVERFLOW
        else:
            coords = children(coords, split)
            depth = depth + split
            level += 1
            continue
        break
    lower = min(best - pr.eps, open_lb.min()) if len(open_lb) else best - pr.eps
    return dict(transform=pr.transform(pose), pose=pose, error=best, lower_bound=float(lower),
                fitness=float((pr.dists(pose[0], pose[1:]) <= p["fitness_radius"]).mean()), status=status, evaluated=ev, survived=sv)
