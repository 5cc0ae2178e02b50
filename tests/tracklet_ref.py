"""The DEFINITION of the KITTI tracklet extraction (csrc/alignnet_crop.hip), NumPy fp64.

A scan point p = (x, y, z) float32 in the Velodyne frame has camera-frame coordinates q = (-y, -z, x) (tp_utils/pointcloud.py:844-846, 859:
R = R1 R2 is a signed permutation, so `pc @ R.T` is exact).  A box b = (bx, by, bz, h, w, l, ry) -- the KITTI label's location, dimensions
and rotation_y -- holds the point iff, with d = q - (bx, by, bz), c = cos ry, s = sin ry (evaluated once, in fp64, by the C library's
cos / sin: math.cos, not np.cos, so that host and restatement hand over the same bits),

    lx = c dx - s dz,   ly = dy,   lz = s dx + c dz,      |lx| <= l / 2,   -h <= ly <= 0,   |lz| <= w / 2.

The box is CLOSED.  This is the convex hull of compute_box_3d's eight corners (:918-940), which the reference tests with scipy's
Delaunay.find_simplex (:769-778); tests/test_tracklet_cpu.py checks the two against each other.  gap = min(l / 2 - |lx|, -ly, ly + h,
w / 2 - |lz|) is the signed distance to the nearest face (>= 0 inside); a point is UNDECIDED when |gap| < 1e-9.  A point with a non-finite
coordinate is in no box.  A crop keeps the scan's order and the points' float32 bits; dz is subtracted from z in ONE float32 subtraction
(`pc2[:, 2] -= z_difference` on a float32 array, as the NumPy of the reference's time evaluates it).  No colour columns."""
import math

import numpy as np

UNDECIDED = 1e-9


def box_frame(points, box):
    """(lx, ly, lz) float64 [n] of float32 points [n, >= 3] (Velodyne frame) in the frame of `box`; every operation rounded as written."""
    p = np.asarray(points)[:, :3].astype(np.float64)
    b = np.asarray(box, np.float64)
    dx, dy, dz = -p[:, 1] - b[0], -p[:, 2] - b[1], p[:, 0] - b[2]
    c, s = math.cos(b[6]), math.sin(b[6])
    with np.errstate(invalid="ignore"):
        return c * dx - s * dz, dy, s * dx + c * dz


def gap(points, box):
    """Signed distance to the nearest face, >= 0 inside; NaN for a non-finite point."""
    b = np.asarray(box, np.float64)
    lx, ly, lz = box_frame(points, box)
    with np.errstate(invalid="ignore"):
        g = np.minimum(np.minimum(b[5] / 2 - np.abs(lx), -ly), np.minimum(ly + b[3], b[4] / 2 - np.abs(lz)))
    finite = np.isfinite(np.asarray(points)[:, :3].astype(np.float64)).all(1)
    return np.where(finite, g, np.nan)


def inside(points, box):
    b = np.asarray(box, np.float64)
    lx, ly, lz = box_frame(points, box)
    finite = np.isfinite(np.asarray(points)[:, :3].astype(np.float64)).all(1)
    with np.errstate(invalid="ignore"):
        return finite & (np.abs(lx) <= b[5] / 2) & (-b[3] <= ly) & (ly <= 0.0) & (np.abs(lz) <= b[4] / 2)


def undecided(points, box):
    with np.errstate(invalid="ignore"):
        return np.abs(gap(points, box)) < UNDECIDED


def crop(scan, box, dz=0.0):
    """float32 [m, 3]: the scan's points inside `box`, in scan order, z (-) float32(dz) in float32."""
    scan = np.asarray(scan, np.float32)
    out = scan[inside(scan, box), :3].copy()
    out[:, 2] = out[:, 2] - np.float32(dz)
    return out


def extract(scans, frames, boxes, dz=None):
    """What Engine.tracklet_extract + tracklet_read return: offsets [B + 1, 2], points1, points2."""
    frames = np.asarray(frames, np.int64).reshape(-1, 2)
    B = len(frames)
    boxes = np.asarray(boxes, np.float64).reshape(B, 2, 7)
    dz = np.zeros((B, 2), np.float32) if dz is None else np.asarray(dz, np.float32).reshape(B, 2)
    parts = ([], [])
    off = np.zeros((B + 1, 2), np.int64)
    for b in range(B):
        for k in range(2):
            parts[k].append(crop(scans[frames[b, k]], boxes[b, k], dz[b, k]))
            off[b + 1, k] = off[b, k] + len(parts[k][-1])
    cat = lambda L: np.concatenate(L, 0) if L else np.zeros((0, 3), np.float32)
    return off, cat(parts[0]), cat(parts[1])


# ---- two WRONG kernels, restated: the tests show that their inputs refuse both ----------------------------------------------------------
def inside_f32(points, box):
    """The membership test with every operation in float32 (box values rounded to float32 first)."""
    p = np.asarray(points, np.float32)[:, :3]
    b = np.asarray(box, np.float64).astype(np.float32)
    dx, dy, dz = -p[:, 1] - b[0], -p[:, 2] - b[1], p[:, 0] - b[2]
    c, s = np.float32(math.cos(box[6])), np.float32(math.sin(box[6]))
    with np.errstate(invalid="ignore"):
        lx, lz = c * dx - s * dz, s * dx + c * dz
        half = np.float32(0.5)
        return np.isfinite(p).all(1) & (np.abs(lx) <= b[5] * half) & (-b[3] <= dy) & (dy <= 0) & (np.abs(lz) <= b[4] * half)


def inside_open(points, box):
    """The open box: < in place of <=."""
    b = np.asarray(box, np.float64)
    lx, ly, lz = box_frame(points, box)
    finite = np.isfinite(np.asarray(points)[:, :3].astype(np.float64)).all(1)
    with np.errstate(invalid="ignore"):
        return finite & (np.abs(lx) < b[5] / 2) & (-b[3] < ly) & (ly < 0.0) & (np.abs(lz) < b[4] / 2)
