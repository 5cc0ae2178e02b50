"""Inputs shared by tests/test_frustum_cpu.py and tests/test_frustum_gpu.py.  A case is a dict: scans (list of float32 [n, stride] in the
Velodyne frame), frames [B, 2], rects [B, 2, 4] float64 = (xmin, ymin, xmax, ymax), proj ([3, 4] or [F, 3, 4]), image ((W, H) or [F, 2]),
dz [B, 2] float32, clip."""
import os
import struct

import numpy as np

from alignnet3d import tracklets as T
from tests import frustum_ref as R
from tests import tracklet_cases as C

# a calibration like KITTI tracking sequence 0000's (P2, R_rect, Tr_velo_cam) and its image size
KITTI = T.Calib(
    np.array([[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01], [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01], [0.0, 0.0, 1.0, 2.745884e-03]]),
    np.array([[9.999239e-01, 9.837760e-03, -7.445048e-03], [-9.869795e-03, 9.999421e-01, -4.278459e-03], [7.402527e-03, 4.351614e-03, 9.999631e-01]]),
    np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03], [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
              [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]]))
KITTI_IMAGE = (1242.0, 375.0)
# every entry a small integer or a power of two, V2C the axis permutation cam = (-y, -z, x): a point (x, -k x / 512, -m x / 512) projects to
# u = 600 + k, v = 180 + m exactly under any operation order wherever the products are exact
DYADIC = T.Calib(np.array([[512.0, 0, 600, 0], [0, 512, 180, 0], [0, 0, 1, 0]]), np.eye(3), np.array([[0.0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0]]))
DYADIC_IMAGE = (1200.0, 360.0)
# a second camera for the frames of one call that differ: another focal length, principal point, mounting and image size
OTHER = T.Calib(np.array([[600.0, 0.0, 480.0, 30.0], [0.0, 610.0, 150.0, -0.5], [0.0, 0.0, 1.0, 0.004]]), KITTI.R0.T.copy(),
                KITTI.V2C + np.array([[0, 0, 0, 0.3], [0, 0, 0, -0.1], [0, 0, 0, 0.2]]))
OTHER_IMAGE = (1000.0, 300.0)
EVERYWHERE = np.array([-1e5, -1e5, 1e5, 1e5])


def calib_text(calib, style="tracking"):
    """A calibration file's text.  tracking: `P2 ...`, R_rect, Tr_velo_cam, Tr_imu_velo (no colons); detection: `P2: ...`, R0_rect,
    Tr_velo_to_cam, and a date line that is no float."""
    row = lambda a: " ".join("%.17e" % v for v in np.ravel(a))   # (KITTI writes twelve digits; seventeen keep every bit of any value)
    if style == "tracking":
        names, sep, extra = ("P2", "R_rect", "Tr_velo_cam"), "", "Tr_imu_velo " + row(np.eye(4)[:3])
    else:
        names, sep, extra = ("P2", "R0_rect", "Tr_velo_to_cam"), ":", "calib_time: 09-Jan-2012 13:57:47"
    lines = ["P0%s %s" % (sep, row(np.eye(4)[:3])), "%s%s %s" % (names[0], sep, row(calib.P)), "%s%s %s" % (names[1], sep, row(calib.R0)),
             "%s%s %s" % (names[2], sep, row(calib.V2C)), extra, ""]
    return "\n".join(lines) + "\n"


def png_header(W, H):
    """The first 33 bytes of a PNG: signature and the IHDR chunk (8-bit RGB; the CRC is not computed: nothing reads it)."""
    return b"\x89PNG\r\n\x1a\n" + struct.pack(">I4sIIBBBBB", 13, b"IHDR", int(W), int(H), 8, 2, 0, 0, 0) + b"\0\0\0\0"


def box_rect(box, M, margin=0.0):
    """The bounding rectangle of the projected corners of a KITTI box (camera frame -> Velodyne by the exact permutation -> M)."""
    corners = np.matmul(T.box_corners(box), T.R).astype(np.float32)
    u, v = R.project(corners, M)
    return np.array([u.min() - margin, v.min() - margin, u.max() + margin, v.max() + margin])


def draw_box(g):
    """A tracked object inside the camera's field of view, 6 .. 50 m ahead."""
    z = g.uniform(6, 50)
    return np.array([z * g.uniform(-0.6, 0.6), g.uniform(1.2, 2.0), z, g.uniform(1.3, 2.0), g.uniform(0.6, 1.9), g.uniform(0.8, 4.6), g.uniform(-np.pi, np.pi)])


def background(g, n):
    """Returns all around the sensor: ahead and behind, inside and outside the image."""
    return np.stack([g.uniform(-40, 60, n), g.uniform(-40, 40, n), g.uniform(-2.5, 3.0, n)], 1).astype(np.float32)


def random_frames(chunk, stride=4, seed=0):
    """Frames of n in {0, 1, 63, 64, 65, C - 1, C, C + 1, 2 C + 1} points, two tracked objects, pairs between consecutive frames (cyclic);
    KITTI-like calibration, the rectangles are the projected boxes.  A third of a frame's points is background."""
    g = np.random.RandomState(seed)
    sizes = [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    F = len(sizes)
    M = T.projection(KITTI)
    obj = np.array([[draw_box(g) for _ in range(2)] for _ in range(F)])
    scans = []
    for f, n in enumerate(sizes):
        which = g.randint(0, 3, n)
        pts = np.zeros((n, 3), np.float32)
        for o in range(2):
            k = np.flatnonzero(which == o)
            pts[k] = C.points_around(g, obj[f, o], len(k), half=2.5)
        k = np.flatnonzero(which == 2)
        pts[k] = background(g, len(k))
        scans.append(C.pad_stride(pts, stride, g))
    frames = np.array([[f, (f + 1) % F] for f in range(F) for _ in range(2)], np.int32)
    rects = np.array([[box_rect(obj[f, o], M), box_rect(obj[(f + 1) % F, o], M)] for f in range(F) for o in range(2)])
    dz = np.zeros((len(frames), 2), np.float32)
    dz[:, 1] = g.uniform(-0.4, 0.4, len(frames)).astype(np.float32)
    return dict(scans=scans, frames=frames, rects=rects, proj=M, image=KITTI_IMAGE, dz=dz, clip=2.0)


def _step(a, up):
    return np.nextafter(np.float32(a), np.float32(np.inf if up else -np.inf))


def half_open_edges(stride=4):
    """The dyadic calibration.  Job 0: the rectangle [640, 700) x [200, 240); job 1: a rectangle beyond the image [0, 1200) x [0, 360) on all
    sides.  Points at x = 8 exactly ON each of the eight edges, and one float32 step of y (or z) to either side of it; points with
    x == clip and x = nextafter(clip) in the image's middle.  expected [2, n] bool comes with the case, from the construction: a point is
    (u, v) in integers plus the sign of the step."""
    rect, image, clip = np.array([640.0, 200.0, 700.0, 240.0]), DYADIC_IMAGE, 2.0
    pts, desc = [], []   # desc: u, du, v, dv, in front
    edges = [(640, 220, 0), (700, 220, 0), (660, 200, 1), (660, 240, 1), (0, 100, 0), (1200, 100, 0), (300, 0, 1), (300, 360, 1)]
    for u, v, axis in edges:
        for s in (0, -1, 1):   # s: the sign of the step in u (axis 0) or v (axis 1)
            y, z = np.float32(-(u - 600) / 64.0), np.float32(-(v - 180) / 64.0)
            if s and axis == 0:
                y = _step(y, s < 0)   # u grows as y falls
            if s and axis == 1:
                z = _step(z, s < 0)
            pts.append([8.0, y, z])
            desc.append((u, s if axis == 0 else 0, v, s if axis == 1 else 0, True))
    pts.append([2.0, 0.0, 0.0]); desc.append((600, 0, 180, 0, False))
    pts.append([_step(2.0, True), 0.0, 0.0]); desc.append((600, 0, 180, 0, True))
    pts.append([_step(2.0, False), 0.0, 0.0]); desc.append((600, 0, 180, 0, False))

    def member(r):
        ge = lambda a, da, lo: a > lo or (a == lo and da >= 0)
        lt = lambda a, da, hi: a < hi or (a == hi and da < 0)
        return [front and ge(u, du, 0) and lt(u, du, image[0]) and ge(v, dv, 0) and lt(v, dv, image[1]) and ge(u, du, r[0]) and lt(u, du, r[2]) and
                ge(v, dv, r[1]) and lt(v, dv, r[3]) for u, du, v, dv, front in desc]

    beyond = np.array([-50.0, -50.0, 1300.0, 400.0])
    scan = np.array(pts, np.float32)
    return dict(scans=[C.pad_stride(scan, stride)], frames=np.zeros((1, 2), np.int32), rects=np.array([[rect, beyond]]), proj=T.projection(DYADIC),
                image=image, dz=np.zeros((1, 2), np.float32), clip=clip, expected=np.array([member(rect), member(beyond)]))


def near_edges(stride=4, seed=7):
    """Edges 1e-6 px on either side of the fp64 u / v of a chosen point, at every one of the eight edges: 16 jobs, `chosen` [16] names each
    job's point and `kept` [16] says on which side of it the edge was put.  Frame 0 (KITTI-like) carries the eight rectangle-edge jobs; the image edges belong to the frame, so W, H (moved next to
    u, v) and u = 0, v = 0 (the calibration shifted: row 0 or 1 of M plus s times row 2 moves u or v by s) have a frame each, all with the
    same scan, and a rectangle that holds everything.  The chosen point of a job is one that the all-float32 projection gets wrong."""
    g = np.random.RandomState(seed)
    M, (W, H), eps = T.projection(KITTI), KITTI_IMAGE, 1e-6
    x = g.uniform(6, 40, 300)
    scan = C.pad_stride(np.stack([x, -x * g.uniform(-0.5, 0.5, 300), -x * g.uniform(-0.12, 0.1, 300) + 0.3], 1), stride, g)
    u, v = R.project(scan, M)
    assert (u > 100).all() and (u < W - 100).all() and (v > 40).all() and (v < H - 40).all()
    projs, images, frames, rects, chosen, kept = [M], [(W, H)], [], [], [], []

    def add(job, frame, keep):
        for c in range(len(scan)):
            rect, m, im = job(c)
            if R.inside(scan[c:c + 1], m, im, rect)[0] != R.inside_f32(scan[c:c + 1], m, im, rect)[0]:
                if frame is None:
                    projs.append(m); images.append(im)
                frames.append(len(projs) - 1 if frame is None else frame); rects.append(rect); chosen.append(c); kept.append(keep)
                return
        raise AssertionError("no point of the scan that the float32 projection gets wrong")

    for side in (-eps, eps):
        add(lambda c: (np.array([u[c] + side, v[c] - 30, u[c] + 40, v[c] + 30]), M, (W, H)), 0, side < 0)   # xmin
        add(lambda c: (np.array([u[c] - 40, v[c] - 30, u[c] + side, v[c] + 30]), M, (W, H)), 0, side > 0)   # xmax
        add(lambda c: (np.array([u[c] - 40, v[c] + side, u[c] + 40, v[c] + 30]), M, (W, H)), 0, side < 0)   # ymin
        add(lambda c: (np.array([u[c] - 40, v[c] - 30, u[c] + 40, v[c] + side]), M, (W, H)), 0, side > 0)   # ymax
        add(lambda c: (EVERYWHERE, M, (u[c] + side, H)), None, side > 0)                                      # W
        add(lambda c: (EVERYWHERE, M, (W, v[c] + side)), None, side > 0)                                      # H

        def shifted(c, row):
            m = M.copy()
            m[row] += (side - (u, v)[row][c]) * M[2]
            return EVERYWHERE, m, (W, H)
        add(lambda c: shifted(c, 0), None, side > 0)                                                          # u = 0
        add(lambda c: shifted(c, 1), None, side > 0)                                                          # v = 0
    F = len(projs)
    return dict(scans=[scan] * F, frames=np.array(frames, np.int32).reshape(-1, 2), rects=np.array(rects).reshape(-1, 2, 4), proj=np.array(projs),
                image=np.array(images), dz=np.zeros((len(frames) // 2, 2), np.float32), clip=2.0, chosen=np.array(chosen), kept=np.array(kept))


def clip_and_behind(stride=4, seed=9):
    """The dyadic calibration (M's last column is zero: p and -p project to the same pixel).  One rectangle; points inside it ahead of the
    clip distance (kept), their mirror images -p (behind the camera, the same pixel), points with 0 < x <= clip inside the rectangle, and
    points with a non-finite coordinate.  expected [n] bool comes with the case."""
    g = np.random.RandomState(seed)
    rect = np.array([500.0, 100.0, 900.0, 300.0])
    n = 60
    k, m = g.randint(-90, 290, n), g.randint(-70, 110, n)   # u = 600 + k in [510, 890), v = 180 + m in [110, 290)
    ahead = np.stack([np.full(n, 8.0), -k / 64.0, -m / 64.0], 1)
    near = np.concatenate([ahead[:20] * (xx / 8.0) for xx in (0.5, 1.0, 2.0)])   # 0 < x <= clip, the same pixels
    bad = ahead[:6].copy()
    bad[0, 0] = np.nan; bad[1, 1] = np.nan; bad[2, 2] = np.nan; bad[3, 0] = np.inf; bad[4, 1] = -np.inf; bad[5, 2] = np.inf
    scan = np.concatenate([ahead, -ahead, near, bad, ahead[:10] * 4.0]).astype(np.float32)
    expected = np.concatenate([np.ones(n, bool), np.zeros(n + len(near) + len(bad), bool), np.ones(10, bool)])
    order = g.permutation(len(scan))
    return dict(scans=[C.pad_stride(scan[order], stride, g)], frames=np.zeros((1, 2), np.int32), rects=np.array([[rect, rect]]), proj=T.projection(DYADIC),
                image=DYADIC_IMAGE, dz=np.zeros((1, 2), np.float32), clip=2.0, expected=expected[order])


def degenerate_rects(stride=4, seed=12):
    """One KITTI-like frame of returns over a field of view wider than the image.  Pair 0: a rectangle that extends beyond the image's right
    and lower edges, and one wholly outside the image (over points that project there); pair 1: xmin > xmax, and zero area."""
    g = np.random.RandomState(seed)
    W, H = KITTI_IMAGE
    x = g.uniform(4, 40, 1500)
    scan = np.stack([x, -x * g.uniform(-1.2, 1.2, 1500), -x * g.uniform(-0.4, 0.4, 1500)], 1)
    rects = np.array([[[W - 150, 200, W + 300, H + 100], [W + 10, 50, W + 300, 300]], [[700, 100, 500, 300], [600, 100, 600, 300]]])
    return dict(scans=[C.pad_stride(scan, stride, g)], frames=np.zeros((2, 2), np.int32), rects=rects, proj=T.projection(KITTI), image=KITTI_IMAGE,
                dz=np.zeros((2, 2), np.float32), clip=2.0)


def job_list_edges(per_pass, stride=4, seed=2):
    """Frame 0 (700 points, KITTI-like) with 2 per_pass + 1 jobs, frame 1 (300 points, the OTHER camera and image size) with per_pass + 1
    jobs, frame 2 with no job, frame 3 empty with two jobs.  Rectangles: 160 x 100 px around the projection of a drawn point."""
    g = np.random.RandomState(seed)
    cams, images = [KITTI, OTHER, KITTI, OTHER], np.array([KITTI_IMAGE, OTHER_IMAGE, KITTI_IMAGE, OTHER_IMAGE])
    proj = np.array([T.projection(c) for c in cams])

    def frame(n):
        x = g.uniform(3, 40, n)
        pts = np.stack([x, -x * g.uniform(-0.9, 0.9, n), -x * g.uniform(-0.3, 0.3, n)], 1)
        pts[::7, 0] = -pts[::7, 0]   # some behind
        return C.pad_stride(pts, stride, g)

    scans = [frame(700), frame(300), frame(90), np.zeros((0, stride), np.float32)]

    def rect(f):
        u, v = g.uniform(0, images[f, 0]), g.uniform(0, images[f, 1])
        return np.array([u - 80, v - 50, u + 80, v + 50])

    pairs = [(0, 1)] * (per_pass + 1) + [(0, 0)] * ((per_pass + 1) // 2) + [(3, 3)]
    frames = np.array(pairs, np.int32)
    rects = np.array([[rect(a), rect(b)] for a, b in pairs])
    dz = np.zeros((len(pairs), 2), np.float32); dz[:, 1] = g.uniform(-0.3, 0.3, len(pairs))
    return dict(scans=scans, frames=frames, rects=rects, proj=proj, image=images, dz=dz, clip=2.0)


def members(case, test=R.inside, frame0_calibration=False):
    """The membership mask of every job (pair-major, cloud-minor) under `test`."""
    proj, image = R.per_frame(case["proj"], case["image"], len(case["scans"]))
    out = []
    for b in range(len(case["frames"])):
        for k in range(2):
            f = case["frames"][b, k]
            c = 0 if frame0_calibration else f
            out.append(test(case["scans"][f], proj[c], image[c], case["rects"][b, k], case["clip"]))
    return out


def undecided_count(case, exact=False):
    """(point tests, undecided ones) of a case; exact: a gap of exactly 0 is decided (exact arithmetic, by the case's construction)."""
    proj, image = R.per_frame(case["proj"], case["image"], len(case["scans"]))
    n_pts = n_und = 0
    for b in range(len(case["frames"])):
        for k in range(2):
            f = case["frames"][b, k]
            gp = R.gap(case["scans"][f], proj[f], image[f], case["rects"][b, k], case["clip"])
            n_pts += len(gp)
            with np.errstate(invalid="ignore"):
                n_und += int(((np.abs(gp) < R.UNDECIDED) & ((gp != 0) if exact else True)).sum())
    return n_pts, n_und


def write_kitti_tree(root, seed=3, n_seq=2, n_frames=4, max_points=3000, image_sizes=((1242, 375), (1224, 370))):
    """tracklet_cases.write_kitti_tree plus what the frustum crop reads: training/calib/%04d.txt (sequence 0 in the tracking files' style,
    sequence 1 in the detection files'), training/image_02/%04d/%06d.png (headers only; sequence 1 has another image size), and labels whose
    2D boxes are the projected 3D boxes (two decimals, as KITTI writes them)."""
    C.write_kitti_tree(root, seed, n_seq, n_frames, max_points)
    for seq in range(n_seq):
        calib = (KITTI, OTHER)[seq % 2]
        M = T.projection(calib)
        os.makedirs(os.path.join(root, "training", "calib"), exist_ok=True)
        with open(os.path.join(root, "training", "calib", "%04d.txt" % seq), "w") as fh:
            fh.write(calib_text(calib, ("tracking", "detection")[seq % 2]))
        os.makedirs(os.path.join(root, "training", "image_02", "%04d" % seq), exist_ok=True)
        for f in range(n_frames):
            with open(os.path.join(root, "training", "image_02", "%04d" % seq, "%06d.png" % f), "wb") as fh:
                fh.write(png_header(*image_sizes[seq % 2]))
        path = os.path.join(root, "training", "label_02", "%04d.txt" % seq)
        lines = []
        for line in open(path):
            t = line.split()
            if t[2] != "DontCare":
                box = np.array([float(x) for x in (t[13], t[14], t[15], t[10], t[11], t[12], t[16])])
                t[6:10] = ["%.2f" % x for x in box_rect(box, M)]   # (a box beside the field of view: a rectangle off the image, an empty crop)
            lines.append(" ".join(t))
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
