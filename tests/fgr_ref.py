"""fp64 NumPy restatement of the fast global registration of csrc/alignnet_globalreg.hip (alignnet_fgr_register*): FGR on FPFH feature
matches of voxel-downsampled clouds, the reference's `o3_gicp_fast` baseline (icp.py:121-143, tp_utils/pointcloud.py:1192-1206).

TEST INFRASTRUCTURE ONLY, and UNPINNED: Open3D (for this baseline a private fork of it: `with_constraint` is not an option of upstream FGR)
is not available next to this stack and the reference holds no code for these steps.  This file restates Open3D 0.7's
FastGlobalRegistration as published (Zhou, Park, Koltun, "Fast Global Registration", ECCV 2016) and IS the definition the kernels are
held to.  Downsample, normals, SPFH / FPFH and the nearest-feature matches are tests/global_reg_ref.py's stages 1-5, imported as they are.

Open3D's, restated:
  the normalisation (each cloud minus its mean, both divided by the largest centred norm; use_absolute_scale = False, so mu starts at 1.0);
  matches both ways and the cross check; the tuple test (ncorr * 100 trials of three correspondences, every pair of edge lengths within
  tuple_scale = 0.95 of each other, strict comparisons, at most maximum_tuple_count = 1000 passing trials, each appending its three
  correspondences, duplicates kept); the Gauss-Newton loop of iteration_number = 64 steps with the line-process weight
  s = (mu / (r.r + mu))^2, Open3D's Jacobian rows ([0, -q_z, q_y, -1, 0, 0] and its cyclic kin), the update T <- Delta T with
  Delta = R_z(x_2) R_y(x_1) R_x(x_0), t = x_3..5; `decrease_mu`: at the end of every iteration k with k % 4 == 0 (so after the first one
  too), while mu > maximum_correspondence_distance, mu /= division_factor -- including Open3D's quirk that mu lives in the normalised frame
  while maximum_correspondence_distance (0.025) is in metres; fewer than 10 correspondences: the identity of the normalised frame; the
  result de-normalised and inverted so that it maps the source onto the target.

This project's own (results are statistically, not numerically, comparable with Open3D's):
  * the trial draws come from the counter generator of the RANSAC stage, draw(seed, stream, trial, k, ncorr), k = 0..2 (Open3D: rand());
  * the cross-checked list holds every mutual pair (i, m_st[i]) once, in ascending i.  Open3D's list holds every mutual pair the same
    number of times (once from each direction) in another order, and it matches the smaller cloud first; the draws being uniform over the
    list, the distribution of a drawn correspondence is the same;
  * the moved target points of an iteration are T q0 computed from the accumulated transform, not Open3D's copy moved step by step by every
    Delta: the same up to rounding, and an iteration is then a function of (T, mu) alone, which is what the GPU test pins on;
  * the solve is a Cholesky factorisation of J^T J in index order; the system is SINGULAR, and the loop stops with the transform so far,
    when a pivot d_k = a_kk - sum_j l_kj^2 is not greater than 1e-12 a_kk (Open3D tests |det| < 1e-6 and then solves by LDL^T);
  * `with_constraint = True` (what all shipped configs set; the fork's code is unknown) is DEFINED as the same loop with the unknowns
    restricted to (x_2, t_x, t_y, t_z): a 4 x 4 system, rotation about z only, like the z-constrained ICP and RANSAC estimates;
  * the inverse of the rigid result is taken in closed form ([R^T, -R^T u]);
  * the score (fitness, inlier rmse) of the result on the downsampled clouds, global_reg_ref.Ransac.score's computation with
    tau = maximum_correspondence_distance, for the log line and the tests;
  * an empty cloud gives the identity, fitness 0 and no correspondences.
`decrease_mu` is an argument everywhere: Open3D's C++ default is true, the 0.7 Python binding the reference calls is remembered to default it
to False, and that cannot be checked here; the command passes False.

Margins of the decisions taken (a test tells a wrong result from a decision within rounding of its boundary):
  matches (both ways)  relative gap between the best and the second-best feature distance (global_reg_ref.matches)
  tuple test           the smallest of |s l_i - l_j| / (l_i + l_j) and |l_j - l_i / s| / (l_i + l_j), s = tuple_scale, over the three edges of
                       every trial drawn up to the stop (inf where both lengths are exactly 0: a repeated index fails on any arithmetic)
  score                |d^2 - tau^2| / tau^2 over the nearest-neighbour distances
The cross check compares integers and has no margin; the Gauss-Newton steps take no decision but the singularity test, which none of the
test inputs comes near (the smallest pivot ratio is returned for that).
"""
import numpy as np
from scipy.spatial import cKDTree

from tests import global_reg_ref as G

DIVISION_FACTOR, MAX_CORR_DIST, ITERATIONS, TUPLE_SCALE, MAX_TUPLES = 1.4, 0.025, 64, 0.95, 1000
MIN_CORRESPONDENCES = 10
PIVOT_EPS = 1e-12


# ---- 1. normalise ----------------------------------------------------------------------------------------------------------------------
def normalise(sp, tp):
    """Returns (means [2, 3], scale): each cloud's mean (summed in index order) and the largest norm of a centred point over both."""
    means = np.zeros((2, 3))
    d2max = 0.0
    for side, P in enumerate((sp, tp)):
        s = np.zeros(3)
        for row in P:
            s += row
        means[side] = s / len(P)
        c = P - means[side]
        d2max = max(d2max, float((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]).max()))
    return means, float(np.sqrt(d2max))


def apply_normalisation(sp, tp, means, scale):
    return (sp - means[0]) / scale, (tp - means[1]) / scale


# ---- 2, 3. matches both ways, cross check ------------------------------------------------------------------------------------------------
def cross_check(m_st, m_ts):
    """The source indices i with m_ts[m_st[i]] == i, ascending."""
    m_st, m_ts = np.asarray(m_st, np.int64), np.asarray(m_ts, np.int64)
    if len(m_st) == 0 or len(m_ts) == 0:
        return np.zeros(0, np.int64)
    return np.nonzero(m_ts[m_st] == np.arange(len(m_st)))[0]


# ---- 4. tuple test -----------------------------------------------------------------------------------------------------------------------
def tuple_test(ns, nt, m_st, cross, seed=0, stream=0, tuple_scale=TUPLE_SCALE, maximum_tuple_count=MAX_TUPLES):
    """ns / nt: the normalised clouds.  Returns dict(ci, cj [3 a] the correspondences of the a accepted trials in trial order, accepted [a]
    their trial indices, trials = the number of trials drawn, margin)."""
    m_st, cross = np.asarray(m_st, np.int64), np.asarray(cross, np.int64)
    ncorr = len(cross)
    z = np.zeros(0, np.int64)
    out = dict(ci=z, cj=z, accepted=z, trials=0, margin=np.inf)
    if ncorr == 0:
        return out
    total = ncorr * 100
    out["trials"] = total
    if maximum_tuple_count <= 0:
        out["trials"] = 0
        return out
    t = np.arange(total)
    r = np.stack([G.draw(seed, stream, t, k, ncorr) for k in range(3)], 1)
    i = cross[r]; j = m_st[i]
    p, q = ns[i], nt[j]
    ok = np.ones(total, bool)
    margin = np.full(total, np.inf)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        li, lj = np.sqrt(G._d2(p[:, a], p[:, b])), np.sqrt(G._d2(q[:, a], q[:, b]))
        ok &= (li * tuple_scale < lj) & (lj < li / tuple_scale)
        with np.errstate(all="ignore"):
            for x, y in ((li * tuple_scale, lj), (lj, li / tuple_scale)):
                margin = np.minimum(margin, np.where((li == 0) & (lj == 0), np.inf, np.abs(x - y) / (li + lj)))
    hits = np.nonzero(ok)[0]
    if len(hits) >= maximum_tuple_count:
        hits = hits[:maximum_tuple_count]
        out["trials"] = int(hits[-1]) + 1
    out.update(ci=i[hits].reshape(-1), cj=j[hits].reshape(-1), accepted=hits, margin=float(margin[: out["trials"]].min()))
    return out


# ---- 5. optimise -------------------------------------------------------------------------------------------------------------------------
def mu_schedule(iteration_number=ITERATIONS, decrease_mu=False, division_factor=DIVISION_FACTOR, maximum_correspondence_distance=MAX_CORR_DIST):
    """mu used by iteration k, k = 0 .. iteration_number - 1 (start 1.0: use_absolute_scale = False)."""
    mu, out = 1.0, np.empty(iteration_number)
    for k in range(iteration_number):
        out[k] = mu
        if decrease_mu and k % 4 == 0 and mu > maximum_correspondence_distance:
            mu /= division_factor
    return out


def delta(x):
    """Open3D's TransformVector6dToMatrix4d: R_z(x2) R_y(x1) R_x(x0), translation x3..5."""
    cx, sx, cy, sy, cz, sz = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    D = np.eye(4)
    D[:3, :3] = Rz @ Ry @ Rx
    D[:3, 3] = x[3:6]
    return D


def cholesky_solve(A, b):
    """x with A x = b by Cholesky in index order, or None when a pivot is not > PIVOT_EPS a_kk.  Returns (x, smallest pivot ratio)."""
    n = len(b)
    L = np.zeros((n, n))
    ratio = np.inf
    for k in range(n):
        d = A[k, k]
        for j in range(k):
            d -= L[k, j] * L[k, j]
        if not d > PIVOT_EPS * A[k, k]:
            return None, 0.0
        ratio = min(ratio, d / A[k, k])
        L[k, k] = np.sqrt(d)
        for i in range(k + 1, n):
            v = A[i, k]
            for j in range(k):
                v -= L[i, j] * L[k, j]
            L[i, k] = v / L[k, k]
    y = np.zeros(n)
    for i in range(n):
        v = b[i]
        for j in range(i):
            v -= L[i, j] * y[j]
        y[i] = v / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        v = y[i]
        for j in range(i + 1, n):
            v -= L[j, i] * x[j]
        x[i] = v / L[i, i]
    return x, ratio


def normal_equations(T, mu, P, Q0):
    """(J^T J [6, 6], J^T r [6]) of one iteration: P [n, 3] the source points of the correspondences, Q0 [n, 3] their target points, both
    normalised; T the transform so far (moves the target points)."""
    q = Q0 @ T[:3, :3].T + T[:3, 3]
    r = P - q
    s = (mu / ((r * r).sum(1) + mu)) ** 2
    n = len(P)
    J = np.zeros((n, 3, 6))
    J[:, 0, 1] = -q[:, 2]; J[:, 0, 2] = q[:, 1]; J[:, 0, 3] = -1.0
    J[:, 1, 2] = -q[:, 0]; J[:, 1, 0] = q[:, 2]; J[:, 1, 4] = -1.0
    J[:, 2, 0] = -q[:, 1]; J[:, 2, 1] = q[:, 0]; J[:, 2, 5] = -1.0
    JTJ = np.einsum("n,nra,nrb->ab", s, J, J)
    JTr = np.einsum("n,nra,nr->a", s, J, r)
    return JTJ, JTr


def gn_step(T, mu, P, Q0, constrained):
    """One Gauss-Newton step.  Returns (T_new or None when the system is singular, x [6], smallest pivot ratio)."""
    JTJ, JTr = normal_equations(T, mu, P, Q0)
    sel = [2, 3, 4, 5] if constrained else [0, 1, 2, 3, 4, 5]
    xs, ratio = cholesky_solve(JTJ[np.ix_(sel, sel)], -JTr[sel])
    if xs is None:
        return None, np.zeros(6), 0.0
    x = np.zeros(6)
    x[sel] = xs
    return delta(x) @ T, x, ratio


def optimise(P, Q0, constrained=True, decrease_mu=False, iteration_number=ITERATIONS, division_factor=DIVISION_FACTOR,
             maximum_correspondence_distance=MAX_CORR_DIST):
    """Returns dict(T [4, 4] normalised frame, maps target onto source; trace [iteration_number, 4, 4] the transform after every iteration --
    after a stop, the transform it stopped with; steps = iterations solved; pivot = the smallest pivot ratio met)."""
    T = np.eye(4)
    trace = np.tile(np.eye(4), (iteration_number, 1, 1))
    steps, pivot = 0, np.inf
    if len(P) >= MIN_CORRESPONDENCES:
        mus = mu_schedule(iteration_number, decrease_mu, division_factor, maximum_correspondence_distance)
        for k in range(iteration_number):
            Tn, _, ratio = gn_step(T, mus[k], P, Q0, constrained)
            if Tn is None:
                trace[k:] = T
                break
            T = Tn
            trace[k] = T
            steps += 1
            pivot = min(pivot, ratio)
    return dict(T=T, trace=trace, steps=steps, pivot=pivot)


def denormalise(Tn, means, scale):
    """The normalised-frame transform (target onto source) in the original frame, inverted: maps the source onto the target."""
    R = Tn[:3, :3]
    u = means[0] + scale * Tn[:3, 3] - R @ means[1]
    T = np.eye(4)
    T[:3, :3] = R.T
    T[:3, 3] = -(R.T @ u)
    return T


# ---- 7. score ------------------------------------------------------------------------------------------------------------------------------
def score(sp, tp, T, tau=MAX_CORR_DIST):
    """(inlier count, fitness, rmse, margin) of T: global_reg_ref.Ransac.score with threshold tau."""
    if len(sp) == 0 or len(tp) == 0:
        return 0, 0.0, 0.0, np.inf
    q = sp @ T[:3, :3].T + T[:3, 3]
    _, j = cKDTree(tp).query(q, k=1, distance_upper_bound=tau * (1 + 1e-6))
    has = j < len(tp)
    d2 = G._d2(q[has], tp[j[has]])
    margin = float((np.abs(d2 - tau * tau) / (tau * tau)).min()) if d2.size else np.inf
    inl = d2 <= tau * tau
    cnt = int(inl.sum())
    return cnt, cnt / float(len(sp)), (float(np.sqrt(d2[inl].sum() / cnt)) if cnt else 0.0), margin


# ---- the whole thing ---------------------------------------------------------------------------------------------------------------------
def register_downsampled(sp, tp, fs, ft, constrained=True, decrease_mu=False, seed=0, stream=0, division_factor=DIVISION_FACTOR,
                         maximum_correspondence_distance=MAX_CORR_DIST, iteration_number=ITERATIONS, tuple_scale=TUPLE_SCALE,
                         maximum_tuple_count=MAX_TUPLES):
    """Steps 1-7 on given downsampled clouds and features.  Returns dict(T, fitness, rmse, correspondences, trials, ...stage outputs)."""
    out = dict(T=np.eye(4), fitness=0.0, rmse=0.0, correspondences=0, trials=0, tuple_margin=np.inf, score_margin=np.inf,
               match_margin=np.zeros(0), rmatch_margin=np.zeros(0))
    if len(sp) == 0 or len(tp) == 0:
        return out
    means, scale = normalise(sp, tp)
    ns, nt = apply_normalisation(sp, tp, means, scale)
    m_st, mm_st = G.matches(fs, ft)
    m_ts, mm_ts = G.matches(ft, fs)
    cross = cross_check(m_st, m_ts)
    tup = tuple_test(ns, nt, m_st, cross, seed, stream, tuple_scale, maximum_tuple_count)
    opt = optimise(ns[tup["ci"]], nt[tup["cj"]], constrained, decrease_mu, iteration_number, division_factor, maximum_correspondence_distance)
    T = denormalise(opt["T"], means, scale)
    cnt, fit, rmse, smargin = score(sp, tp, T, maximum_correspondence_distance)
    out.update(T=T, fitness=fit, rmse=rmse, correspondences=len(tup["ci"]), trials=tup["trials"], tuple_margin=tup["margin"], score_margin=smargin,
               match_margin=mm_st, rmatch_margin=mm_ts, means=means, scale=scale, matches=m_st, rmatches=m_ts, cross=cross, tuples=tup, opt=opt)
    return out


def front_end(pc):
    """Stages 1-4 of tests/global_reg_ref.py on one raw cloud: (downsampled points, FPFH)."""
    ds = G.voxel_downsample(pc)
    nr = G.normals(ds["points"])
    sp = G.spfh(ds["points"], nr["normals"])
    return ds["points"], G.fpfh(ds["points"], sp["spfh"])["fpfh"]


def fgr_register(src, dst, front=None, **kw):
    """The whole pipeline on one pair of raw clouds; `front` = ((sp, fs), (tp, ft)) reuses a front end already computed."""
    (sp, fs), (tp, ft) = front if front is not None else (front_end(src), front_end(dst))
    return register_downsampled(sp, tp, fs, ft, **kw)
