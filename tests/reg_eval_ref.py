"""The definition of alignnet_evaluate_registration* (csrc/alignnet_icp.hip, icp_kernel<.., kEval = true>) in NumPy fp64, and the inputs of its tests
(tests/test_reg_eval_cpu.py, tests/test_reg_eval_gpu.py).  TEST INFRASTRUCTURE ONLY.

Per pair, ONE correspondence step at the given 4x4 transform T (Open3D's evaluate_registration and get_information_matrix_from_point_clouds):
  p = R s + t for every source point s; its nearest target q_j by brute force, equal squared distances going to the lowest index j;
  an inlier when dist2 <= threshold^2 (closed, as the ICP loop has it);
  fitness = inliers / n1;  rmse = sqrt(sum of the inliers' dist2 / inliers), 0 without inliers;
  correspondences [n1] = j for an inlier, -1 otherwise;
  information [6, 6] = sum over the inliers of G^T G, where with (x, y, z) = q_j - centre (the TARGET point; centre None = the origin)
      G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]]      parameters: rotation x, y, z; translation x, y, z.
  An empty source or target: fitness 0, rmse 0, all correspondences -1, the zero matrix.

Margins are tests/icp_scan_ref.py's: a source point is UNDECIDED when its two smallest distinct squared distances, or its squared distance and
threshold^2, lie closer than UNDECIDED (1000) x b64 -- what two correct fp64 evaluations may differ by.  At most POINT_CAP (1e-3) of a case's points may
be undecided; the committed seeds below have none (tests/test_reg_eval_cpu.py asserts it), so every comparison is on every point.
"""
import numpy as np

from tests.icp_scan_ref import LDS_BUDGET, POINT_CAP, evaluate_with_margins, rigid_about, size_pair   # noqa: F401 (POINT_CAP, LDS_BUDGET: the tests')


def information_matrix(q):
    """sum of G^T G over the rows (x, y, z) of q [n, 3] (float64)."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    G = np.zeros((len(q), 3, 6))
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    G[:, 0, 1], G[:, 0, 2], G[:, 0, 3] = z, -y, 1.0
    G[:, 1, 0], G[:, 1, 2], G[:, 1, 4] = -z, x, 1.0
    G[:, 2, 0], G[:, 2, 1], G[:, 2, 5] = y, -x, 1.0
    return np.einsum("nki,nkj->ij", G, G)


def evaluate_registration(src, dst, T, threshold, centre=None, exact=False):
    """The call on one pair.  Returns dict(fitness, rmse, correspondences [n1] int32, information [6, 6], undecided [n1] bool, dist2 [n1]).
    exact=True: every operation is exact on this input (dyadic coordinates, identity T), nothing is undecided."""
    src = np.asarray(src, np.float32).reshape(-1, 3).astype(np.float64)
    dst = np.asarray(dst, np.float32).reshape(-1, 3).astype(np.float64)
    n1, n2 = len(src), len(dst)
    if n1 == 0 or n2 == 0:
        return dict(fitness=0.0, rmse=0.0, correspondences=np.full(n1, -1, np.int32), information=np.zeros((6, 6)), undecided=np.zeros(n1, bool),
                    dist2=np.full(n1, np.inf))
    e = evaluate_with_margins(src, dst, T, float(threshold), exact=exact)
    corr = np.where(e["inlier"], e["index"], -1).astype(np.int32)
    c = np.zeros(3) if centre is None else np.asarray(centre, np.float64).reshape(3)
    return dict(fitness=e["fitness"], rmse=e["rmse"], correspondences=corr, information=information_matrix(dst[e["index"][e["inlier"]]] - c),
                undecided=e["undecided"], dist2=e["best"])


# ---- inputs: every generator returns a list of cases dict(name, src, dst, T, threshold, centre, exact) ------------------------------------------
def _case(name, src, dst, T, threshold, centre=None, exact=False):
    return dict(name=name, src=np.ascontiguousarray(src, np.float32).reshape(-1, 3), dst=np.ascontiguousarray(dst, np.float32).reshape(-1, 3),
                T=np.asarray(T, np.float64), threshold=float(threshold), centre=centre, exact=exact)


SIZES_N1 = (0, 1, 255, 256, 257, 1025)
SIZES_N2 = (0, 1, 5)
SIZES_TAIL = (LDS_BUDGET, LDS_BUDGET + 1)   # 4266: the last target the scan stages in LDS; 4267: one target behind the stage
SIZE_SEED = 5


def size_cases():
    """n1 x n2 over the edges of the kernel's loops (1024 threads, 256 quads per round of the scan), both empty kinds, and two target sizes at the end
    of the scan's LDS stage with source 0 sitting on the LAST target (index 4266 comes from the fp64 tail)."""
    out = []
    for n1 in SIZES_N1:
        for n2 in SIZES_N2 + SIZES_TAIL:
            if n2 > 5 and n1 != 257:
                continue
            if n1 == 0 or n2 == 0:
                rng = np.random.default_rng(SIZE_SEED + n1 + n2)
                out.append(_case("size_%d_%d" % (n1, n2), rng.uniform(-1, 1, (n1, 3)), rng.uniform(-1, 1, (n2, 3)), np.eye(4), 0.1))
                continue
            src, dst, T = size_pair(n1, n2, SIZE_SEED + 7 * n1 + n2, duplicates=False)
            if n2 > 5:
                src = src.copy()
                src[0] = ((dst[-1].astype(np.float64) + [0.003, -0.002, 0.001] - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
            out.append(_case("size_%d_%d" % (n1, n2), src, dst, T, 0.1))
    return out


def _lattice(h, shape, seed):
    g = [np.arange(k, dtype=np.float64) * h for k in shape]
    lat = np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
    return lat[np.random.default_rng(seed).permutation(len(lat))]


def threshold_edge_case():
    """Lattice target (spacing 2^-4), sources beyond its +x face at EXACTLY the threshold 2^-4 from their only candidate (inliers: <=), one float32
    ulp inside (inliers) and one ulp outside (not).  Identity T, dyadic coordinates: every operation is exact.  Returns (case, points per group)."""
    h = 2.0 ** -4
    lat = _lattice(h, (6, 6, 4), 11)
    face = lat[lat[:, 0] == 5 * h]
    on = (face + [h, 0.0, 0.0]).astype(np.float32)
    inside, outside = on.copy(), on.copy()
    inside[:, 0] = np.nextafter(on[:, 0], np.float32(-np.inf))
    outside[:, 0] = np.nextafter(on[:, 0], np.float32(np.inf))
    return _case("threshold_edge", np.concatenate([on, inside, outside]), lat, np.eye(4), h, exact=True), len(on)


def tie_case():
    """Sources at the centres of the lattice's unit squares in the xy plane: FOUR targets at the same exact distance h / sqrt(2) each; the lattice is
    permuted, so the lowest index is wherever the permutation put it.  Identity T, dyadic coordinates: exact."""
    h = 2.0 ** -3
    lat = _lattice(h, (7, 7, 3), 12)
    c = np.arange(6, dtype=np.float64) * h + h / 2
    src = np.stack(np.meshgrid(c, c, np.arange(3, dtype=np.float64) * h, indexing="ij"), -1).reshape(-1, 3)
    return _case("ties4", src, lat, np.eye(4), h, exact=True)


FAR_SEED = 3
FAR_CENTRE = np.array([4000.0, -500.0, 30.0])   # 4 km from the origin


def far_cases():
    """One pair 4 km out, a general small rigid T about the clouds' centre: without a centre (Open3D's matrix, entries of 1e10) and about the target's mean."""
    rng = np.random.default_rng(FAR_SEED)
    dst = (rng.uniform(-1.5, 1.5, (900, 3)) + FAR_CENTRE).astype(np.float32)
    T = rigid_about(FAR_CENTRE, (0.004, -0.003, 0.02), (0.05, -0.03, 0.01))
    picks = rng.integers(len(dst), size=700)
    p = dst[picks].astype(np.float64) + rng.normal(0, 0.03, (700, 3))
    src = ((p - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    centre = dst.astype(np.float64).mean(0)
    return [_case("far_origin", src, dst, T, 0.1), _case("far_centred", src, dst, T, 0.1, centre=centre)]


THRESHOLDS = (1e-3, 0.02, 0.1, 5.0)
THRESHOLD_SEED = 21


def threshold_cases():
    src, dst, T = size_pair(300, 400, THRESHOLD_SEED, duplicates=False)
    return [_case("threshold_%g" % t, src, dst, T, t) for t in THRESHOLDS]


BATCH_SEED = 40
BATCH_PAIRS = 40


def batch_cases():
    """40 pairs of mixed sizes at ONE threshold (a call has one), among them an empty source, an empty target and both empty; every third with a centre."""
    rng = np.random.default_rng(BATCH_SEED)
    out = []
    for b in range(BATCH_PAIRS):
        n1, n2 = int(rng.integers(1, 700)), int(rng.integers(1, 900))
        if b == 5:
            n1 = 0
        if b == 17:
            n2 = 0
        if b == 29:
            n1 = n2 = 0
        if n1 == 0 or n2 == 0:
            src, dst, T = rng.uniform(-1, 1, (n1, 3)), rng.uniform(-1, 1, (n2, 3)), np.eye(4)
        else:
            src, dst, T = size_pair(n1, n2, BATCH_SEED + 1 + b, duplicates=False)
        centre = rng.uniform(-5, 5, 3) if b % 3 == 0 else np.zeros(3)
        out.append(_case("batch_%d" % b, src, dst, T, 0.05, centre=centre))
    return out


def all_cases():
    return size_cases() + [threshold_edge_case()[0], tie_case()] + far_cases() + threshold_cases() + batch_cases()
