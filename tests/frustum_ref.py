"""The DEFINITION of the image-frustum crop (csrc/alignnet_crop.hip, alignnet_tracklet_extract_frustum), NumPy fp64.

The reference's extract_pointcloud(tracklet, from_bbox2d=True, calib) (tp_utils/pointcloud.py:840-869) keeps every LiDAR return whose
image projection falls inside the label's 2D box: extract_pc_in_box2d (:794-801) -> get_lidar_in_image_fov (:781-791) ->
Calibration.project_velo_to_image (:41-202).  Restated:

    M = P R4 V4 [3, 4]      R4 = R0 padded to 4 x 4, V4 = V2C padded to 4 x 4; np.matmul(P, np.matmul(R4, V4)), evaluated ONCE on the host
                            (the "do matrix multiplication only once" the reference leaves as a TODO); its bits go to the device
    w_i = ((M[i,0] x + M[i,1] y) + M[i,2] z) + M[i,3]      x, y, z the float32 point widened to fp64; every product and sum rounded as written
    u = w_0 / w_2,  v = w_1 / w_2

A point is kept for the image size (W, H), the clip distance `clip` (the reference's 2.0) and a rectangle (xmin, ymin, xmax, ymax) iff its
coordinates are finite, x > clip, 0 <= u < W, 0 <= v < H, xmin <= u < xmax and ymin <= v < ymax: HALF-OPEN intervals, the reference's.  A
comparison with a NaN or infinite u / v is false (w_2 == 0: in no crop); the sign of w_2 is not tested, as in the reference.
gap = min(u, W - u, v, H - v, u - xmin, xmax - u, v - ymin, ymax - v, x - clip); a point is UNDECIDED when |gap| < 1e-9
(tracklet_ref.UNDECIDED); a NaN gap counts as decided outside.  A crop keeps the scan's order and the points' float32 bits; dz is
subtracted from z in ONE float32 subtraction, as in the box crop.  No colour columns."""
import numpy as np

from tests.tracklet_ref import UNDECIDED


def projection(P, R0, V2C):
    R4, V4 = np.eye(4), np.eye(4)
    R4[:3, :3] = np.asarray(R0, np.float64).reshape(3, 3)
    V4[:3, :4] = np.asarray(V2C, np.float64).reshape(3, 4)
    return np.matmul(np.asarray(P, np.float64).reshape(3, 4), np.matmul(R4, V4))


def project(points, M, dtype=np.float64):
    """(u, v) [n] of float32 points [n, >= 3]; every operation in `dtype`, rounded as written."""
    p = np.asarray(points, np.float32)[:, :3].astype(dtype)
    M = np.asarray(M, np.float64).reshape(3, 4).astype(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        w = [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)]
        return w[0] / w[2], w[1] / w[2]


def _finite(points):
    return np.isfinite(np.asarray(points, np.float32)[:, :3]).all(1)


def inside(points, M, image, rect, clip=2.0):
    u, v = project(points, M)
    x = np.asarray(points, np.float32)[:, 0].astype(np.float64)
    (W, H), (xmin, ymin, xmax, ymax) = image, rect
    with np.errstate(invalid="ignore"):
        return (_finite(points) & (x > clip) & (0 <= u) & (u < W) & (0 <= v) & (v < H) & (xmin <= u) & (u < xmax) & (ymin <= v) & (v < ymax))


def gap(points, M, image, rect, clip=2.0):
    """Signed distance to the nearest of the nine decisions (pixels, and metres for the clip), >= 0 inside; NaN where u / v are."""
    u, v = project(points, M)
    x = np.asarray(points, np.float32)[:, 0].astype(np.float64)
    (W, H), (xmin, ymin, xmax, ymax) = image, rect
    with np.errstate(invalid="ignore"):
        g = np.stack([u, W - u, v, H - v, u - xmin, xmax - u, v - ymin, ymax - v, x - clip])
        return np.where(np.isnan(g).any(0), np.nan, g.min(0))


def undecided(points, M, image, rect, clip=2.0):
    with np.errstate(invalid="ignore"):
        return np.abs(gap(points, M, image, rect, clip)) < UNDECIDED


def crop(scan, M, image, rect, dz=0.0, clip=2.0, test=inside):
    """float32 [m, 3]: the scan's points the test keeps, in scan order, z (-) float32(dz) in float32."""
    scan = np.asarray(scan, np.float32)
    out = scan[test(scan, M, image, rect, clip), :3].copy()
    out[:, 2] = out[:, 2] - np.float32(dz)
    return out


def per_frame(proj, image, F):
    """proj [3, 4] / [12] / [F, 3, 4] and image (W, H) / [F, 2] as [F, 3, 4] and [F, 2]: Engine.tracklet_extract_frustum's broadcasting."""
    proj, image = np.asarray(proj, np.float64), np.asarray(image, np.float64)
    proj = np.broadcast_to(proj.reshape(1, 3, 4), (F, 3, 4)) if proj.size == 12 else proj.reshape(F, 3, 4)
    image = np.broadcast_to(image.reshape(1, 2), (F, 2)) if image.ndim == 1 else image.reshape(F, 2)
    return proj, image


def extract(scans, frames, rects, proj, image, dz=None, clip=2.0, test=inside, frame0_calibration=False):
    """What Engine.tracklet_extract_frustum + tracklet_read return: offsets [B + 1, 2], points1, points2."""
    frames = np.asarray(frames, np.int64).reshape(-1, 2)
    B = len(frames)
    rects = np.asarray(rects, np.float64).reshape(B, 2, 4)
    dz = np.zeros((B, 2), np.float32) if dz is None else np.asarray(dz, np.float32).reshape(B, 2)
    proj, image = per_frame(proj, image, len(scans))
    parts = ([], [])
    off = np.zeros((B + 1, 2), np.int64)
    for b in range(B):
        for k in range(2):
            f = frames[b, k]
            c = 0 if frame0_calibration else f
            parts[k].append(crop(scans[f], proj[c], image[c], rects[b, k], dz[b, k], clip, test))
            off[b + 1, k] = off[b, k] + len(parts[k][-1])
    cat = lambda L: np.concatenate(L, 0) if L else np.zeros((0, 3), np.float32)
    return off, cat(parts[0]), cat(parts[1])


# ---- five WRONG kernels, restated: the tests show that their inputs refuse every one (the fifth is extract(frame0_calibration=True)) --------
def inside_f32(points, M, image, rect, clip=2.0):
    """The projection with every operation in float32 (M rounded to float32 first); the comparisons as in the definition."""
    u, v = project(points, M, np.float32)
    u, v = u.astype(np.float64), v.astype(np.float64)
    x = np.asarray(points, np.float32)[:, 0].astype(np.float64)
    (W, H), (xmin, ymin, xmax, ymax) = image, rect
    with np.errstate(invalid="ignore"):
        return (_finite(points) & (x > clip) & (0 <= u) & (u < W) & (0 <= v) & (v < H) & (xmin <= u) & (u < xmax) & (ymin <= v) & (v < ymax))


def inside_closed(points, M, image, rect, clip=2.0):
    """Closed upper edges: <= in place of <."""
    u, v = project(points, M)
    x = np.asarray(points, np.float32)[:, 0].astype(np.float64)
    (W, H), (xmin, ymin, xmax, ymax) = image, rect
    with np.errstate(invalid="ignore"):
        return (_finite(points) & (x > clip) & (0 <= u) & (u <= W) & (0 <= v) & (v <= H) & (xmin <= u) & (u <= xmax) & (ymin <= v) & (v <= ymax))


def inside_noclip(points, M, image, rect, clip=2.0):
    """No clip test: points behind the camera project into the image too."""
    u, v = project(points, M)
    (W, H), (xmin, ymin, xmax, ymax) = image, rect
    with np.errstate(invalid="ignore"):
        return (_finite(points) & (0 <= u) & (u < W) & (0 <= v) & (v < H) & (xmin <= u) & (u < xmax) & (ymin <= v) & (v < ymax))


def inside_noimage(points, M, image, rect, clip=2.0):
    """No image-bounds test: the rectangle alone."""
    u, v = project(points, M)
    x = np.asarray(points, np.float32)[:, 0].astype(np.float64)
    xmin, ymin, xmax, ymax = rect
    with np.errstate(invalid="ignore"):
        return _finite(points) & (x > clip) & (xmin <= u) & (u < xmax) & (ymin <= v) & (v < ymax)
