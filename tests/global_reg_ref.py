"""fp64 NumPy / SciPy restatement of the global registration of csrc/alignnet_globalreg.hip (alignnet_global_register*): RANSAC on FPFH
feature matches of voxel-downsampled clouds, the reference's `o3_gicp` baseline (icp.py:85-143).

TEST INFRASTRUCTURE ONLY, and UNPINNED: Open3D is not available next to this stack and the reference holds no code for these steps (it calls
Open3D).  This file restates Open3D's published algorithms of the 0.7 line (voxel_down_sample, estimate_normals, compute_fpfh_feature,
registration_ransac_based_on_feature_matching with the edge-length and distance checkers) and IS the definition the kernels are held to.
Two points are this project's own, so results are statistically, not numerically, comparable with Open3D's: the output order of the
downsample (ascending (ix, iy, iz)) and the counter-based generator of the RANSAC draws (`draw`).  Radius and threshold tests are taken on
squared distances (d^2 <= r^2), as the ICP kernel does.

Every stage is callable on given upstream outputs and returns, for every discrete decision it takes, its MARGIN, so that a test can tell a
wrong result from a decision that sits within rounding of its boundary:
  floor()           distance of the pre-floor value to the nearest bin edge, as a fraction of the bin width
  neighbour sets    |d^2 - r^2| / r^2 over the candidates, and the relative gap between the max_nn-th and the next d^2
  normals           (l1 - l0) / l2 of the covariance's ascending eigenvalues l0 <= l1 <= l2 (the gap that conditions the eigenvector), and |n . z|
  swap test (SPFH)  | acos|a1| - acos|a2| |
  matches           relative gap between the best and the second-best feature distance; target rows equal to the best one count as one
                    candidate, whose lowest index wins (`matches`)
  RANSAC            the smallest relative margin over every comparison taken for the pair (a < 0.9 b, d^2 > tau^2, d^2 <= tau^2)
"""
import functools

import numpy as np
from scipy.spatial import cKDTree

VOXEL = 0.05
TAU = 1.5 * VOXEL
GOLD = np.uint64(0x9E3779B97F4A7C15)


def _d2(a, b):
    d = b - a
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


# ---- 1. voxel downsample ---------------------------------------------------------------------------------------------------------------
def voxel_downsample(pc, v=VOXEL):
    """pc [n, 3] float32.  Returns dict(points [m, 3] f64, voxels [m, 3] int, counts [m], margin [n] per input point)."""
    pc = np.asarray(pc, np.float32).reshape(-1, 3)
    if len(pc) == 0:
        return dict(points=np.zeros((0, 3)), voxels=np.zeros((0, 3), np.int64), counts=np.zeros(0, np.int64), margin=np.zeros(0))
    m = pc.min(0).astype(np.float64) - v / 2
    pre = (pc.astype(np.float64) - m) / v
    idx = np.floor(pre).astype(np.int64)
    margin = np.minimum(pre - np.floor(pre), np.floor(pre) + 1 - pre).min(1)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    order = np.argsort(key, kind="stable")            # ascending (ix, iy, iz), then ascending point index
    ks = key[order]
    head = np.r_[True, ks[1:] != ks[:-1]]
    seg = np.cumsum(head) - 1
    sums = np.zeros((seg[-1] + 1, 3))
    np.add.at(sums, seg, pc[order].astype(np.float64))   # sequential: ascending point index inside a voxel
    counts = np.bincount(seg)
    return dict(points=sums / counts[:, None], voxels=idx[order][head], counts=counts, margin=margin)


# ---- 2. neighbour sets -----------------------------------------------------------------------------------------------------------------
def neighbours(points, radius, max_nn):
    """Hybrid search.  Returns (I, J, D, count [m], margin [m]): flattened pairs (point, neighbour, d^2) with the point itself included,
    per point in ascending (d^2, index) order when max_nn cut the set and ascending index otherwise."""
    m = len(points)
    if m == 0:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0), z, np.zeros(0)
    r2 = radius * radius
    tree = cKDTree(points)
    lists = tree.query_ball_point(points, radius * (1 + 1e-6))
    I = np.repeat(np.arange(m), [len(l) for l in lists])
    J = np.concatenate([np.sort(np.asarray(l, np.int64)) for l in lists])
    D = _d2(points[I], points[J])
    margin = np.full(m, np.inf)
    np.minimum.at(margin, I, np.abs(D - r2) / r2)
    keep = D <= r2
    I, J, D = I[keep], J[keep], D[keep]
    count = np.bincount(I, minlength=m)
    if (count > max_nn).any():
        starts = np.r_[0, np.cumsum(count)]
        sel = np.ones(len(I), bool)
        perm = np.arange(len(I))
        for i in np.nonzero(count > max_nn)[0]:
            s, e = starts[i], starts[i + 1]
            o = np.lexsort((J[s:e], D[s:e]))
            perm[s:e] = s + o
            sel[s + max_nn:e] = False
            ds = D[s:e][o]
            margin[i] = min(margin[i], (ds[max_nn] - ds[max_nn - 1]) / max(ds[max_nn], 1e-300))
        I, J, D = I[perm][sel], J[perm][sel], D[perm][sel]
        count = np.minimum(count, max_nn)
    return I, J, D, count, margin


# ---- 3. normals ------------------------------------------------------------------------------------------------------------------------
def normals(points, radius=2 * VOXEL, max_nn=30):
    """Returns dict(normals [m, 3], nbr_margin, gap, nz): gap / nz are inf where the normal is the default (fewer than 3 neighbours)."""
    m = len(points)
    I, J, D, count, nmargin = neighbours(points, radius, max_nn)
    out = np.tile([0.0, 0.0, 1.0], (m, 1))
    gap, nz = np.full(m, np.inf), np.full(m, np.inf)
    starts = np.r_[0, np.cumsum(count)]
    for i in np.nonzero(count >= 3)[0]:
        q = points[J[starts[i]:starts[i + 1]]]
        K = len(q)
        mean = np.zeros(3)
        for row in q:
            mean += row
        mean /= K
        c = q - mean
        cov = np.zeros((3, 3))
        for row in c:
            cov += np.outer(row, row)
        cov /= K
        w, v = np.linalg.eigh(cov)
        n = v[:, 0]
        nn = np.linalg.norm(n)
        n = n / nn if nn > 0 else np.array([0.0, 0.0, 1.0])
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        nz[i] = abs(n[2])
        out[i] = -n if n[2] < 0 else n
    return dict(normals=out, nbr_margin=nmargin, gap=gap, nz=nz)


# ---- 4. SPFH / FPFH --------------------------------------------------------------------------------------------------------------------
def _bin(v):
    """clamp(floor(v), 0, 10) and the margin to the nearest INTERIOR bin edge (1 .. 10: values beyond the ends are clamped into the end bins)."""
    b = np.where(v >= 0, np.where(v >= 11, 10, np.floor(np.where(np.isfinite(v), v, 0.0))), 0).astype(np.int64)
    edge = np.clip(np.round(v), 1, 10)
    return b, np.abs(v - edge)


def pair_bins(p1, n1, p2, n2):
    """Vectorised pair features -> (bins [k, 3] in 0..32, margin [k])."""
    d = p2 - p1
    f3 = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    with np.errstate(all="ignore"):
        a1 = (n1 * d).sum(1) / f3
        a2 = (n2 * d).sum(1) / f3
        c1, c2 = np.arccos(np.abs(a1)), np.arccos(np.abs(a2))
        swap = c1 > c2
        mswap = np.where(np.abs(a1) == np.abs(a2), np.inf, np.abs(c1 - c2))
        mswap = np.where(np.isnan(mswap), 0.0, mswap)
        n1c = np.where(swap[:, None], n2, n1); n2c = np.where(swap[:, None], n1, n2)
        d = np.where(swap[:, None], -d, d)
        f2 = np.where(swap, -a2, a1)
        vv = np.cross(d, n1c)
        vn = np.sqrt(vv[:, 0] * vv[:, 0] + vv[:, 1] * vv[:, 1] + vv[:, 2] * vv[:, 2])
        vv = vv / vn[:, None]
        w = np.cross(n1c, vv)
        f1 = (vv * n2c).sum(1)
        f0 = np.arctan2((w * n2c).sum(1), (n1c * n2c).sum(1))
    zero = (f3 == 0) | (vn == 0)
    f0, f1, f2 = (np.where(zero, 0.0, f) for f in (f0, f1, f2))
    mswap = np.where(f3 == 0, np.inf, mswap)
    b0, m0 = _bin(11.0 * (f0 + np.pi) / (2.0 * np.pi))
    b1, m1 = _bin(11.0 * (f1 + 1.0) / 2.0)
    b2, m2 = _bin(11.0 * (f2 + 1.0) / 2.0)
    return np.stack([b0, 11 + b1, 22 + b2], 1), np.minimum(np.minimum(m0, m1), np.minimum(m2, mswap))


def spfh(points, nrm, radius=5 * VOXEL, max_nn=100):
    """Returns dict(spfh [m, 33], nbr_margin [m], margin [m] = the smallest bin / swap margin over the point's pairs)."""
    m = len(points)
    I, J, D, count, nmargin = neighbours(points, radius, max_nn)
    out = np.zeros((m, 33))
    margin = np.full(m, np.inf)
    other = I != J
    I, J = I[other], J[other]
    if len(I):
        bins, mg = pair_bins(points[I], nrm[I], points[J], nrm[J])
        np.minimum.at(margin, I, mg)
        cnt = np.zeros((m, 33))
        for k in range(3):
            np.add.at(cnt, (I, bins[:, k]), 1.0)
        with np.errstate(all="ignore"):
            out = np.where(count[:, None] >= 2, cnt * (100.0 / (count[:, None] - 1.0)), 0.0)
    return dict(spfh=out, nbr_margin=nmargin, margin=margin)


def fpfh(points, sp, radius=5 * VOXEL, max_nn=100):
    """Returns dict(fpfh [m, 33], nbr_margin [m])."""
    m = len(points)
    I, J, D, count, nmargin = neighbours(points, radius, max_nn)
    use = (I != J) & (D > 0) & (count[I] >= 2)
    acc = np.zeros((m, 33))
    np.add.at(acc, I[use], sp[J[use]] / D[use, None])
    for g in range(3):
        s = acc[:, g * 11:(g + 1) * 11].sum(1)
        scale = np.where(s != 0, 100.0 / np.where(s != 0, s, 1.0), 1.0)
        acc[:, g * 11:(g + 1) * 11] *= scale[:, None]
    return dict(fpfh=acc + sp, nbr_margin=nmargin)


# ---- 5. matches ------------------------------------------------------------------------------------------------------------------------
def matches(fs, ft, with_ties=False):
    """Nearest target feature of every source feature (lowest index wins a tie).  Returns (index [ms], margin [ms]), and with_ties also
    tied [ms] bool.

    Target rows that are EQUAL to the nearest row, entry for entry, form its group: the same operations on the same values give the same
    distance on any arithmetic, so among them the tie is decided and the lowest index of the group is the answer (an isolated point's
    all-zero row, and the rows of points with one neighbour, which hold nothing but 0 and 100, repeat across a cloud).  The margin is the
    relative gap between the group's distance and the best distance over the rows outside the group, inf when every row is in it; tied =
    the group has more than one member.  Without equal rows this is the gap between the best and the second-best distance."""
    ms, mt = len(fs), len(ft)
    idx, margin, tied = np.zeros(ms, np.int64), np.full(ms, np.inf), np.zeros(ms, bool)
    if mt and ms:
        _, gid = np.unique(ft, axis=0, return_inverse=True)
        gid = gid.reshape(-1)
        first = np.full(gid.max() + 1, mt, np.int64)
        np.minimum.at(first, gid, np.arange(mt))
        size = np.bincount(gid)
        for s in range(0, ms, 64):
            d = ((fs[s:s + 64, None, :] - ft[None, :, :]) ** 2).sum(-1)
            g = gid[d.argmin(1)]
            idx[s:s + 64] = first[g]
            tied[s:s + 64] = size[g] > 1
            other = np.where(gid[None, :] == g[:, None], np.inf, d).min(1)
            with np.errstate(invalid="ignore"):
                margin[s:s + 64] = np.where(np.isinf(other), np.inf, (other - d.min(1)) / np.maximum(other, 1e-300))
    return (idx, margin, tied) if with_ties else (idx, margin)


# ---- 6. RANSAC -------------------------------------------------------------------------------------------------------------------------
def draw(seed, stream, it, k, n):
    """Index into n source points of draw k of iteration it (arrays broadcast)."""
    assert 0 <= int(stream) < (1 << 24) and np.all(np.asarray(it) < (1 << 38))
    with np.errstate(over="ignore"):
        ctr = (np.uint64(stream) << np.uint64(40)) | (np.asarray(it, np.uint64) << np.uint64(2)) | np.asarray(k, np.uint64)
        x = np.asarray([seed % (1 << 64)], np.uint64) * GOLD + ctr
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        z = x ^ (x >> np.uint64(31))
        return (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _estimate(s, t, constrained):
    """s, t [h, 4, 3] -> (T [h, 4, 4], rank margin [h])."""
    h = len(s)
    mp, mq = s.mean(1), t.mean(1)
    pc, qc = s - mp[:, None, :], t - mq[:, None, :]
    T = np.tile(np.eye(4), (h, 1, 1))
    rank = np.full(h, np.inf)
    if constrained:
        sxy = (pc[:, :, 0] * qc[:, :, 1] - pc[:, :, 1] * qc[:, :, 0]).sum(1)
        sxx = (pc[:, :, 0] * qc[:, :, 0] + pc[:, :, 1] * qc[:, :, 1]).sum(1)
        th = np.arctan2(sxy, sxx)
        T[:, 0, 0] = np.cos(th); T[:, 0, 1] = -np.sin(th); T[:, 1, 0] = np.sin(th); T[:, 1, 1] = np.cos(th)
    elif h:
        S = np.einsum("hki,hkj->hij", qc, pc) / 4.0
        U, sv, Vt = np.linalg.svd(S)
        sign = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
        U[:, :, 2] *= sign[:, None]
        T[:, :3, :3] = U @ Vt
        rank = np.where(sv[:, 0] > 0, sv[:, 1] / np.where(sv[:, 0] > 0, sv[:, 0], 1.0), 0.0)
    T[:, :3, 3] = mq - np.einsum("hij,hj->hi", T[:, :3, :3], mp)
    return T, rank


class Ransac:
    """RANSAC of one pair on given downsampled clouds and matches."""

    def __init__(self, sp, tp, match, constrained=True, seed=0, stream=0):
        self.sp, self.tp, self.match = np.asarray(sp, np.float64), np.asarray(tp, np.float64), np.asarray(match, np.int64)
        self.constrained, self.seed, self.stream = constrained, seed, stream
        self.tree = cKDTree(self.tp) if len(self.tp) else None
        self.margin = np.inf

    def prechecks(self, its, track=True):
        """its: array of iteration indices.  Returns (passes [k] bool, T [k, 4, 4]); track: fold the comparisons' margins into self.margin."""
        keep = self.margin
        its = np.asarray(its, np.int64)
        n = len(self.sp)
        idx = np.stack([draw(self.seed, self.stream, its, k, n) for k in range(4)], 1)
        s, t = self.sp[idx], self.tp[self.match[idx]]
        ok = np.ones(len(its), bool)
        for j in range(4):
            for k in range(j + 1, 4):
                a, b = np.sqrt(_d2(s[:, j], s[:, k])), np.sqrt(_d2(t[:, j], t[:, k]))
                ok &= ~((a < 0.9 * b) | (b < 0.9 * a))
                for x, y in ((a, 0.9 * b), (b, 0.9 * a)):
                    with np.errstate(all="ignore"):
                        mg = np.where(x == y, np.inf, np.abs(x - y) / (x + y))
                    self.margin = min(self.margin, mg.min() if len(mg) else np.inf)
        T = np.tile(np.eye(4), (len(its), 1, 1))
        sel = np.nonzero(ok)[0]
        Ts, rank = _estimate(s[sel], t[sel], self.constrained)
        q = np.einsum("hij,hkj->hki", Ts[:, :3, :3], s[sel]) + Ts[:, None, :3, 3]
        d2 = _d2(t[sel], q)
        if d2.size:
            self.margin = min(self.margin, (np.abs(d2 - TAU * TAU) / (TAU * TAU)).min())
        good = (d2 <= TAU * TAU).all(1)
        T[sel] = Ts
        ok[sel] = good
        self._rank = dict(zip(its[sel].tolist(), rank.tolist()))
        if not track:
            self.margin = keep
        return ok, T

    def score(self, T, track=True):
        """(inlier count, fitness, rmse) of T: nearest downsampled target point of every transformed source point, within TAU."""
        q = self.sp @ T[:3, :3].T + T[:3, 3]
        _, j = self.tree.query(q, k=1, distance_upper_bound=TAU * (1 + 1e-6))
        has = j < len(self.tp)
        d2 = _d2(q[has], self.tp[j[has]])
        if track and d2.size:
            self.margin = min(self.margin, (np.abs(d2 - TAU * TAU) / (TAU * TAU)).min())
        inl = d2 <= TAU * TAU
        cnt = int(inl.sum())
        return cnt, cnt / float(len(self.sp)), (float(np.sqrt(d2[inl].sum() / cnt)) if cnt else 0.0)

    def run(self, max_iteration=4000000, max_validation=500, chunk=1 << 16):
        """Returns dict(T, fitness, rmse, iterations, validations, win, margin)."""
        best = dict(T=np.eye(4), fitness=0.0, rmse=0.0, iterations=0, validations=0, win=-1)
        if len(self.sp) < 4 or len(self.tp) < 4 or max_validation <= 0:
            best["margin"] = np.inf
            return best
        cnt_best, validated, it0 = 0, 0, 0
        best["iterations"] = max_iteration
        while it0 < max_iteration:
            its = np.arange(it0, min(max_iteration, it0 + chunk))
            ok, T = self.prechecks(its, track=False)
            hits = np.nonzero(ok)[0]
            stop = None
            for h in hits:
                cnt, fit, rmse = self.score(T[h])
                if not self.constrained and not self._rank[int(its[h])] > 1e-9:
                    self.margin = 0.0     # correspondences of rank <= 1: the rotation about their line is free
                if cnt > cnt_best or (cnt == cnt_best and rmse < best["rmse"]):
                    cnt_best = cnt
                    best.update(T=T[h].copy(), fitness=fit, rmse=rmse, win=int(its[h]))
                validated += 1
                if validated == max_validation:
                    stop = int(its[h])
                    break
            # margins of the pre-checks that were taken: the iterations up to the stop
            self.prechecks(its if stop is None else np.arange(it0, stop + 1))
            if stop is not None:
                best["iterations"] = stop + 1
                break
            it0 += chunk
        best["validations"] = validated
        best["margin"] = self.margin
        return best


def front_end(pc):
    """Stages 1-4 on one raw cloud: dict(ds, normals, spfh, fpfh) of the stages' outputs."""
    ds = voxel_downsample(pc)
    nr = normals(ds["points"])
    sp = spfh(ds["points"], nr["normals"])
    return dict(ds=ds, normals=nr, spfh=sp, fpfh=fpfh(ds["points"], sp["spfh"]))


def global_register(src, dst, constrained=True, seed=0, stream=0, max_iteration=4000000, max_validation=500, stages=None):
    """The whole pipeline on one pair of raw clouds (`stages`: their front ends, when already computed).  Returns the RANSAC dict plus the
    stage outputs, the matches, their margins and which of them are ties between equal target rows."""
    st = list(stages) if stages is not None else [front_end(src), front_end(dst)]
    m, mm, tied = matches(st[0]["fpfh"]["fpfh"], st[1]["fpfh"]["fpfh"], with_ties=True)
    res = Ransac(st[0]["ds"]["points"], st[1]["ds"]["points"], m, constrained, seed, stream).run(max_iteration, max_validation)
    res.update(stages=st, matches=m, match_margin=mm, match_tied=tied)
    return res


# ---- test clouds -----------------------------------------------------------------------------------------------------------------------
_BOXES = (((0.0, 0.0, 0.0), (4.2, 1.7, 0.7)), ((0.7, 0.1, 0.7), (2.2, 1.5, 0.6)), ((3.5, 0.15, 0.7), (0.5, 0.5, 0.4)))


def _surface(rng, n):
    """n points on the surfaces of three joined boxes of about car size (body, cabin set back, a small box on one side of the bonnet:
    no rotational or mirror symmetry)."""
    areas = np.array([2 * (sx * sy + sy * sz + sx * sz) for _, (sx, sy, sz) in _BOXES])
    which = rng.choice(len(_BOXES), n, p=areas / areas.sum())
    out = np.empty((n, 3))
    for b, (o, size) in enumerate(_BOXES):
        sel = np.nonzero(which == b)[0]
        sx, sy, sz = size
        fa = np.array([sy * sz, sy * sz, sx * sz, sx * sz, sx * sy, sx * sy])
        face = rng.choice(6, len(sel), p=fa / fa.sum())
        u = rng.uniform(0, 1, (len(sel), 3))
        axis = face // 2
        u[np.arange(len(sel)), axis] = face % 2
        out[sel] = np.asarray(o) + u * np.asarray(size)
    return out


def _planted_motion(rng, ctr, max_shift, yaw_only, tilt):
    """(R, t) of x = R p + t: a yaw anywhere in (-pi, pi] (plus tilts up to `tilt` rad when not yaw_only) about `ctr`, and up to max_shift in
    x and y."""
    yaw = rng.uniform(-np.pi, np.pi)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    if not yaw_only:
        a, b = rng.uniform(-tilt, tilt, 2)
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        R = R @ Ry @ Rx
    return R, ctr - R @ ctr + np.r_[rng.uniform(-max_shift, max_shift, 2), 0.0]


def car_pairs(n_pairs, seed, n_points=4500, noise=0.01, max_shift=0.6, yaw_only=True, tilt=0.05, scale=1.0, offset=None):
    """Targets: n_points on the surface of the object with clipped noise, somewhere within +-15 m (moved by `offset` before the rounding to
    float32, when given); sources: a 70 % subset of them moved by
    a yaw anywhere in (-pi, pi] (plus tilts up to `tilt` rad when not yaw_only) and up to max_shift in x and y; `scale` shrinks the object (fewer points then cover it as densely).  Returns (sources, targets,
    truths): truth maps the source onto the target."""
    rng = np.random.default_rng(seed)
    src, dst, truth = [], [], []
    for _ in range(n_pairs):
        x = _surface(rng, n_points) * scale + rng.uniform(-15, 15, 3)
        x = x + np.clip(rng.normal(0, noise, x.shape), -2 * noise, 2 * noise)
        if offset is not None:
            x = x + np.asarray(offset, np.float64)
        R, t = _planted_motion(rng, x.mean(0), max_shift, yaw_only, tilt)
        keep = rng.permutation(n_points)[: int(n_points * 0.7)]
        p = (x[keep] - t) @ R          # x = R p + t
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
        src.append(p.astype(np.float32)); dst.append(x.astype(np.float32)); truth.append(T)
    return src, dst, truth


# ---- the inputs the GPU tests run on (tests/test_global_reg_gpu.py), shared with the CPU checks of their margins -------------------------
TEST_ITERATIONS, TEST_VALIDATIONS = 200000, 50
UNDECIDED, UNDECIDED_GAP, UNDECIDED_RANSAC, SKIP_CAP = 1e-9, 1e-6, 1e-10, 1e-3


def gpu_test_pairs(constrained):
    """8 pairs per estimate form: 1800 points on the object at scale 0.3 (1.26 m long: every surface voxel of 5 cm is hit, so the normals'
    neighbourhoods hold about a dozen points), yaw anywhere, with small tilts for the full-rotation form."""
    return car_pairs(8, seed=11 if constrained else 12, n_points=1800, scale=0.3, max_shift=0.3, yaw_only=constrained)


def default_pair():
    """The pair run at Open3D's defaults (4,000,000 iterations / 500 validations)."""
    s, d, t = car_pairs(1, seed=21, n_points=2000, scale=0.3, max_shift=0.3)
    return s[0], d[0], t[0]


def large_pair():
    """A target that downsamples to more points than the LDS-resident validation grid holds (6314); the source is half of the object."""
    s, d, t = car_pairs(1, seed=31, n_points=16000, scale=0.9, max_shift=0.3)
    return s[0][s[0][:, 0] < np.median(s[0][:, 0])], d[0], t[0]


# ---- inputs that reach what the surfaces above never do: both max_nn cuts, the candidate spill, isolated points, tied matches, a grid that
# ---- has to grow, the voxel-span limit and a frame far from the origin (measured figures: tests/test_global_reg_cpu.py) ------------------
VOLUME_ITERATIONS, VOLUME_VALIDATIONS = 20000, 20
WIDE_ITERATIONS, WIDE_VALIDATIONS = 20000, 5
CAND_LDS = 320                  # kCandLds of csrc/alignnet_globalreg.hip: a wave's candidates beyond these are ranked from HBM
MAX_GRID_CELLS = 32768          # kMaxCells
VOLUME_SEED = {True: 66, False: 62}
CLUTTER_SEED, FAR_SEED, WIDE_SEED = 71, 81, 91
FAR_OFFSET = (4000.0, -3000.0, 50.0)
WIDE_X = 100000.0               # the accepted span ends at 2^21 * VOXEL = 104,857.6 m


def _frozen(*arrays):
    """The arrays, read-only: what a cached generator hands out is shared."""
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def volume_pair(constrained=True):
    """A filled box: 24,000 points uniform in 0.8 x 0.6 x 0.45 m, the source an exact 70 % subset under a yaw anywhere (small tilts too for
    the full-rotation form) and up to 0.3 m of shift.  The 5 cm voxel means of a volume hold about 45 points within 0.10 m and 520 within
    0.25 m: the normals are cut to their 30 nearest, the features to their 100 nearest, and more than kCandLds candidates are ranked.
    The box is nearly symmetric: no motion recovery is claimed on it.  Returns (source, target, truth)."""
    rng = np.random.default_rng(VOLUME_SEED[constrained])
    n = 24000
    x = rng.uniform(0, 1, (n, 3)) * np.array([0.8, 0.6, 0.45]) + rng.uniform(-15, 15, 3)
    R, t = _planted_motion(rng, x.mean(0), 0.3, constrained, 0.05)
    keep = rng.permutation(n)[: int(n * 0.7)]
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return _frozen(((x[keep] - t) @ R).astype(np.float32), x.astype(np.float32), T)


@functools.lru_cache(maxsize=None)
def clutter_pair():
    """The object of gpu_test_pairs among 48 stray returns.  The sites lie within +-8 m of the object's centre, at least 2 m from it and 1 m
    from each other; a third are single points (no neighbour: default normal, all-zero feature rows), a third carry a second point 0.064 m
    away (one neighbour within both radii), a third one 0.173 m away (none within 0.10, one within 0.25).  All clutter is in both clouds, the
    object's points are subsampled to 70 % in the source.  The zero rows and the one-neighbour rows (nothing but 0 and 100) repeat, so the
    matches hold exact ties; the cloud spans some 15 m, so the validation grid's cell has to grow.  Returns (source, target, truth)."""
    rng = np.random.default_rng(CLUTTER_SEED)
    n = 1800
    obj = _surface(rng, n) * 0.3 + rng.uniform(-15, 15, 3)
    obj = obj + np.clip(rng.normal(0, 0.01, obj.shape), -0.02, 0.02)
    ctr = obj.mean(0)
    sites = []
    while len(sites) < 48:
        c = ctr + rng.uniform(-8, 8, 3)
        if np.linalg.norm(c - ctr) >= 2.0 and all(np.linalg.norm(c - o) >= 1.0 for o in sites):
            sites.append(c)
    clutter = []
    for k, c in enumerate(sites):
        clutter.append(c)
        if k % 3:
            u = rng.normal(size=3)
            clutter.append(c + u / np.linalg.norm(u) * (0.064 if k % 3 == 1 else 0.173))
    clutter = np.asarray(clutter)
    R, t = _planted_motion(rng, ctr, 0.3, True, 0.0)
    keep = rng.permutation(n)[: int(n * 0.7)]
    x = np.concatenate([obj, clutter])
    p = (np.concatenate([obj[keep], clutter]) - t) @ R
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    return _frozen(p.astype(np.float32), x.astype(np.float32), T)


def far_pair():
    """The object of gpu_test_pairs in a frame (4000, -3000, 50) m from the origin, where float32 coordinates are 2.4e-4 m apart: raw points
    then sit ON voxel edges in exact arithmetic (an offset of an odd multiple of 0.125 m from the cloud's minimum is representable, and
    0.125 + 0.025 is three voxels), and the floor is decided by the rounding of 0.05 and 0.025 alone -- in fp64 by hundreds of times the
    rounding of the one inexact operation, the division; in fp32 not at all."""
    s, d, t = car_pairs(1, seed=FAR_SEED, n_points=1800, scale=0.3, max_shift=0.3, offset=FAR_OFFSET)
    return s[0], d[0], t[0]


def wide_pair():
    """far_pair's recipe near the origin, plus one point WIDE_X m away in x, the same in both clouds: 2,000,000 voxels wide, inside the limit
    of 2^21, and the validation grid's cell grows from 0.075 m to metres before its cells fit."""
    s, d, t = car_pairs(1, seed=WIDE_SEED, n_points=1800, scale=0.3, max_shift=0.3)
    far = (d[0].astype(np.float64).mean(0) + [WIDE_X, 0.0, 0.0]).astype(np.float32)[None]
    return np.concatenate([s[0], far]), np.concatenate([d[0], far]), t[0]


def too_wide_cloud():
    """Two points 110,000 m apart: more than 2^21 voxels of 0.05 m."""
    return np.array([[0.0, 0.0, 0.0], [110000.0, 0.0, 0.0]], np.float32)


def radius_counts(points, radius):
    """Points within `radius` of every point (itself included), before any max_nn cut."""
    return neighbours(points, radius, len(points) + 1)[3]


def grid_cells(points, tau=TAU):
    """Cells of a uniform grid of edge 1.001 tau over the points: what the validation grid would need before its cell grows."""
    e = np.floor((points.max(0) - points.min(0)) / (1.001 * tau)) + 1
    return int(e[0]) * int(e[1]) * int(e[2])


NEW_PAIRS = ("volume", "volume_full", "clutter", "far", "wide")


def new_pair(name):
    """(source, target, truth) of one of NEW_PAIRS."""
    return {"volume": lambda: volume_pair(True), "volume_full": lambda: volume_pair(False), "clutter": clutter_pair, "far": far_pair,
            "wide": wide_pair}[name]()


@functools.lru_cache(maxsize=None)
def new_pair_stages(name):
    """The restatement's front end of both clouds of one of NEW_PAIRS, computed once per process: shared by the CPU tests, which only read it."""
    s, d, _ = new_pair(name)
    return [front_end(s), front_end(d)]


def stage_shares(st, match_margin):
    """Share of undecided entries per stage, from stage outputs of `global_register` (or the same structure built on device outputs)."""
    cat = lambda f: np.concatenate([f(s) for s in st])
    return dict(
        voxel=float((cat(lambda s: s["ds"]["margin"]) < UNDECIDED).mean()),
        normals=float(cat(lambda s: (s["normals"]["nbr_margin"] < UNDECIDED) | (s["normals"]["gap"] < UNDECIDED_GAP) | (s["normals"]["nz"] < UNDECIDED)).mean()),
        spfh=float(cat(lambda s: (s["spfh"]["nbr_margin"] < UNDECIDED) | (s["spfh"]["margin"] < UNDECIDED)).mean()),
        fpfh=float(cat(lambda s: s["fpfh"]["nbr_margin"] < UNDECIDED).mean()),
        matches=float((match_margin < UNDECIDED).mean()))
