"""fp64 restatement of MULTI-SCALE (coarse-to-fine) ICP, the definition of alignnet_icp_multiscale_register* (csrc/alignnet_multiscale.hip) -- Open3D's
multi_scale_icp: both clouds voxel-downsampled per level, the existing ICP run level by level from the transform of the level before.  TEST
INFRASTRUCTURE ONLY.  Nothing is restated twice: the level cloud is tests/global_reg_ref.py::voxel_downsample at the level's voxel size followed by
the rounding of the mean to float32 (the ICP kernels take float32 clouds), the loops are tests/icp_scan_ref.py::icp_with_margins (tests/icp_full_ref.py
::icp_p2point's loop with margins), tests/icp_plane_ref.py::icp_plane and tests/icp_generalized_ref.py::icp_generalized, imported as they are.

A call has L levels, 1 <= L <= 8, and three lists of L: voxel_sizes[l] (> 0: downsample at that edge; <= 0: the raw cloud), radii[l] (> 0) and
its[l] (>= 0; 0 evaluates only).  Level l runs on (source_l, target_l) from T_{l-1} (T_{-1} = the init); normals of a level are taken on that level's
clouds within normal_radius (a scalar or a list of L).  Result: the last level's transform, fitness and inlier rmse (on its clouds, at its radius),
iterations per level, level sizes.  An empty level cloud: the level returns its input transform and 0 iterations, as an empty cloud does today."""
import numpy as np

from tests import global_reg_ref as G
from tests import icp_full_ref as F
from tests import icp_generalized_ref as GEN
from tests import icp_plane_ref as P
from tests import icp_scan_ref as S

MAX_LEVELS = 8
FACE = 1e-9               # bin widths: a point nearer than this to a voxel face is undecided (tests/test_global_reg_gpu.py's threshold for this stage)
FACE_CAP, FACE_REF_CAP = 1e-3, 1e-4   # share of a cloud's points that may be: in a GPU test; on the committed inputs, by the restatement alone
MEAN_TOL = 1e-12          # relative, fp64 means (the existing bar of this stage)


def level_cloud(pc, v):
    """The cloud a level with voxel size v runs on, float32 [m, 3]; v <= 0: pc itself (Open3D's rule)."""
    pc = np.asarray(pc, np.float32).reshape(-1, 3)
    if not v > 0:
        return pc
    return G.voxel_downsample(pc, v)["points"].astype(np.float32)


def pyramid(pc, voxel_sizes):
    """Per level dict(points f32 [m, 3], means f64, voxels, counts, margin [n]); a level with voxel <= 0: the raw cloud, voxels None."""
    pc = np.asarray(pc, np.float32).reshape(-1, 3)
    out = []
    for v in voxel_sizes:
        if not v > 0:
            out.append(dict(points=pc, means=pc.astype(np.float64), voxels=None, counts=np.ones(len(pc), np.int64), margin=np.full(len(pc), 0.5)))
            continue
        d = G.voxel_downsample(pc, v)
        out.append(dict(points=d["points"].astype(np.float32), means=d["points"], voxels=d["voxels"], counts=d["counts"], margin=d["margin"]))
    return out


def undecided_share(pc, v):
    """Share of the cloud's points within FACE bin widths of a voxel face at voxel size v."""
    pc = np.asarray(pc, np.float32).reshape(-1, 3)
    return float((G.voxel_downsample(pc, v)["margin"] < FACE).mean()) if len(pc) and v > 0 else 0.0


def check_schedule(voxel_sizes, radii, its):
    L = len(voxel_sizes)
    if not (1 <= L <= MAX_LEVELS) or len(radii) != L or len(its) != L:
        raise ValueError("1 <= L <= %d levels, three lists of L" % MAX_LEVELS)
    if any(not r > 0 for r in radii) or any(i < 0 for i in its):
        raise ValueError("radii > 0, its >= 0")
    return L


def run_level(src, dst, T, radius, its, estimate, normal_radius, constrained):
    """One level on given clouds through the existing restatement of `estimate`.  Returns (T, fitness, rmse, iterations, undecided, entries): undecided
    of `entries` decisions lay within the restatement's margins."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    if estimate == "point":
        T, fit, rmse, k, und, evals = S.icp_with_margins(src, dst, T, radius, its, constrained)
        return T, fit, rmse, k, und, max(evals * len(src), 1)
    fn = P.icp_plane if estimate == "plane" else GEN.icp_generalized
    info = {}
    T, fit, rmse, k, und = fn(src, dst, T, radius=radius, normal_radius=normal_radius, its=its, constrained=constrained, info=info)
    return T, fit, rmse, k, und, max(info.get("evaluations", 0) * len(src) + len(dst) + (len(src) if estimate == "generalized" else 0), 1)


def icp_multiscale(src, dst, init, voxel_sizes, radii, its, estimate="point", normal_radius=0.3, constrained=True):
    """Returns dict(transform, fitness, rmse, iterations [L], level_sizes [L, 2], undecided, entries, levels: the transforms after every level)."""
    L = check_schedule(voxel_sizes, radii, its)
    nr = np.broadcast_to(np.asarray(normal_radius, np.float64).reshape(-1), (L,))
    T = np.array(init, np.float64).reshape(4, 4)
    fit = rmse = 0.0
    iters, sizes, levels, und, ent = [], [], [], 0, 0
    for l in range(L):
        s, d = level_cloud(src, voxel_sizes[l]), level_cloud(dst, voxel_sizes[l])
        T, fit, rmse, k, u, e = run_level(s, d, T, radii[l], its[l], estimate, nr[l], constrained)
        iters.append(k); sizes.append((len(s), len(d))); levels.append(T.copy()); und += u; ent += e
    return dict(transform=T, fitness=fit, rmse=rmse, iterations=np.array(iters), level_sizes=np.array(sizes), undecided=und, entries=ent, levels=levels)


def icp_single(src, dst, init, radius, its, estimate="point", normal_radius=0.3, constrained=True):
    """The single-scale restatement a one-level call with voxel <= 0 must equal bit for bit: (T, fitness, rmse, iterations)."""
    if estimate == "point":
        return F.icp_p2point(src, dst, init, radius, its, with_constraint=constrained)
    fn = P.icp_plane if estimate == "plane" else GEN.icp_generalized
    return fn(src, dst, init, radius=radius, normal_radius=normal_radius, its=its, constrained=constrained)[:4]


# ---- two wrong pyramids (tests/test_icp_multiscale_cpu.py: what the GPU test's bars must catch) ----------------------------------------------------
def level_cloud_fp32_sum(pc, v):
    """The mean summed in float32 (ascending point index) instead of fp64."""
    pc = np.asarray(pc, np.float32).reshape(-1, 3)
    d = G.voxel_downsample(pc, v)
    m = pc.min(0).astype(np.float64) - v / 2
    idx = np.floor((pc.astype(np.float64) - m) / v).astype(np.int64)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    order = np.argsort(key, kind="stable")
    ends = np.cumsum(d["counts"])
    out = np.zeros((len(ends), 3), np.float32)
    for q, (b, e) in enumerate(zip(ends - d["counts"], ends)):
        s = np.zeros(3, np.float32)
        for i in order[b:e]:
            s = (s + pc[i]).astype(np.float32)
        out[q] = s / np.float32(e - b)
    return out


def level_cloud_origin_at_min(pc, v):
    """The origin at the minimum, without - v / 2."""
    pc = np.asarray(pc, np.float32).reshape(-1, 3)
    m = pc.min(0).astype(np.float64)
    idx = np.floor((pc.astype(np.float64) - m) / v).astype(np.int64)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.r_[True, ks[1:] != ks[:-1]]
    seg = np.cumsum(head) - 1
    sums = np.zeros((seg[-1] + 1, 3))
    np.add.at(sums, seg, pc[order].astype(np.float64))
    return (sums / np.bincount(seg)[:, None]).astype(np.float32)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
CAR_VOXELS = (0.4, 0.2, 0.1, 0.05)
FAR = np.array([4000.0, -3000.0, 50.0])


def car_scan(seed=3, dist=8.0):
    """A noisy scan pair of the built-in car (tests/icp_plane_ref.py::car_pair): (src, dst, truth)."""
    return P.car_pair(dist, seed)


# Voxel sizes for clouds at FAR.  There float32 x and y are multiples of 2^-12 m, and a point k steps above the minimum sits EXACTLY on a voxel face when
# k = (2 j + 1) v 2^11 is an integer: with v = 0.05 that is every k = 512 (2 t + 1), two in a thousand points whatever the seed (0.4: 2.4e-4, 0.2: 5e-4).
# With v = n / 1000, n odd and no multiple of 5, the first such k is 256 n steps = n / 16 m away: rarer than FACE_REF_CAP on a car.
FAR_VOXELS = (0.403, 0.203, 0.103, 0.057)


def far_pair(seed=4, dist=25.0):
    """The same kind of pair 4 km out: both clouds and the truth moved by FAR, coordinates rounded to float32 there.  (Seed and distance were
    chosen by undecided_share: tests/test_icp_multiscale_cpu.py asserts it; the target of (5, 10.0) has one point in 8,498 on a face at 0.057.)"""
    src, dst, truth = P.car_pair(dist, seed)
    s = (src.astype(np.float64) + FAR).astype(np.float32)
    d = (dst.astype(np.float64) + FAR).astype(np.float32)
    M = np.eye(4); M[:3, 3] = FAR
    return s, d, M @ truth @ np.linalg.inv(M)


def lattice(n=4000, seed=11):
    """Coordinates that are multiples of 2^-4 in [0, 4): at voxel 2^-3 every operation is exact (minimum 0 or a multiple of 2^-4, origin minus 2^-4,
    quotient a multiple of 1/2) and most points lie exactly on a voxel face -- the closed lower face of floor decides them."""
    rng = np.random.default_rng(seed)
    pc = (rng.integers(0, 64, (n, 3)) / 16.0).astype(np.float32)
    pc[0] = 0.0   # the minimum is the origin of the lattice
    return pc


def on_face_share(pc, v):
    pc = np.asarray(pc, np.float32).reshape(-1, 3)
    pre = (pc.astype(np.float64) - (pc.min(0).astype(np.float64) - v / 2)) / v
    return float((pre == np.floor(pre)).any(1).mean())


def far_cloud():
    """One 8,383-point cloud at FAR for the pyramid stage."""
    return far_pair(5, 10.0)[0]


SMALL_PAIRS = ((6, 40.0), (4, 25.0), (3, 14.5))   # (seed, distance) of the small car pairs: 481 / 1,324 / 3,569 source points


def disturbed_init(src, truth, seed, degrees=4.0, shift=0.12):
    """A start the levels have something to do from: the truth turned about z through the source's centre and shifted (tests/icp_plane_ref.py)."""
    return P.disturbed(truth, (np.asarray(src, np.float64).mean(0) @ truth[:3, :3].T + truth[:3, 3]) if len(src) else np.zeros(3), degrees, shift, seed)
