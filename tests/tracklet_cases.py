"""Inputs shared by tests/test_tracklet_cpu.py and tests/test_tracklet_gpu.py.  A case is a dict: scans (list of float32 [n, stride] in the
Velodyne frame), frames [B, 2], boxes [B, 2, 7] float64 = (x, y, z, h, w, l, ry) in the camera frame, dz [B, 2] float32."""
import numpy as np


def to_velodyne(q):
    """Camera-frame points (fp64) as float32 Velodyne points: p = (qz, -qx, -qy)."""
    q = np.asarray(q, np.float64)
    return np.stack([q[:, 2], -q[:, 0], -q[:, 1]], 1).astype(np.float32)


def pad_stride(scan, stride, g=None):
    """[n, 3] -> [n, stride]: stride 4 adds a reflectance column (noise: it must not be read as a coordinate)."""
    scan = np.asarray(scan, np.float32).reshape(-1, 3)
    if stride == 3:
        return scan
    refl = (g or np.random.RandomState(0)).uniform(0, 1, (len(scan), stride - 3)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([scan, refl], 1))


def draw_box(g, offset=0.0):
    return np.array([g.uniform(-20, 20) + offset, g.uniform(0.8, 2.2), g.uniform(4, 60) + offset, g.uniform(1.3, 2.0), g.uniform(0.6, 1.9),
                     g.uniform(0.8, 4.6), g.uniform(-np.pi, np.pi)])


def points_around(g, box, n, half=4.0):
    """n float32 Velodyne points in a cube of 2 * half metres around the box's middle."""
    mid = box[:3] - [0, box[3] / 2, 0]
    return to_velodyne(mid + g.uniform(-half, half, (n, 3)))


def random_frames(chunk, stride=4, seed=0):
    """Frames of n in {0, 1, 63, 64, 65, C - 1, C, C + 1, 2 C + 1} points, two tracked objects, pairs between consecutive frames (cyclic)."""
    g = np.random.RandomState(seed)
    sizes = [0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    F = len(sizes)
    obj = np.array([[draw_box(g) for _ in range(2)] for _ in range(F)])
    scans = []
    for f, n in enumerate(sizes):
        which = g.randint(0, 2, n)
        pts = np.zeros((n, 3), np.float32)
        for o in range(2):
            k = np.flatnonzero(which == o)
            pts[k] = points_around(g, obj[f, o], len(k), half=2.5)
        scans.append(pad_stride(pts, stride, g))
    frames = np.array([[f, (f + 1) % F] for f in range(F) for _ in range(2)], np.int32)
    boxes = np.array([[obj[f, o], obj[(f + 1) % F, o]] for f in range(F) for o in range(2)])
    dz = np.zeros((len(frames), 2), np.float32)
    dz[:, 1] = g.uniform(-0.4, 0.4, len(frames)).astype(np.float32)
    return dict(scans=scans, frames=frames, boxes=boxes, dz=dz)


def closed_faces(stride=4):
    """ry = 0, centre and half extents powers of two: every product and difference of the test is exact (with or without fused multiply-add).
    Points on every face, edge and corner and in the middle (27, all inside the CLOSED box), and for each of them one float32 step outwards
    (outside) and inwards (inside) along every axis in which it sits on the boundary.  expected [n] bool comes with the case."""
    box = np.array([8.0, 4.0, 16.0, 2.0, 2.0, 4.0, 0.0])   # x in [6, 10], y in [2, 4], z in [15, 17]: no coordinate near 0, where a float32 step is lost in q - b
    lo, hi = np.array([6.0, 2.0, 15.0], np.float32), np.array([10.0, 4.0, 17.0], np.float32)
    mid = (lo + hi) / 2
    pts, expect = [], []
    for ix in range(3):
        for iy in range(3):
            for iz in range(3):
                sel = (ix, iy, iz)
                q = np.array([(lo[a], mid[a], hi[a])[sel[a]] for a in range(3)], np.float32)
                pts.append(q.copy()); expect.append(True)
                for a in range(3):
                    if sel[a] == 1:
                        continue
                    away = np.float32(-np.inf if sel[a] == 0 else np.inf)
                    for toward, ins in ((away, False), (-away, True)):
                        s = q.copy()
                        s[a] = np.nextafter(q[a], toward)
                        pts.append(s); expect.append(ins)
    q = np.array(pts, np.float32)
    scan = np.stack([q[:, 2], -q[:, 0], -q[:, 1]], 1)   # exact: sign changes only
    return dict(scans=[pad_stride(scan, stride)], frames=np.zeros((1, 2), np.int32), boxes=np.array([[box, box]]), dz=np.zeros((1, 2), np.float32),
                expected=np.array(expect))


def far_frame(stride=4, seed=5):
    """One frame 5 km from the origin, where a float32 step is 0.5 mm: box faces lie BETWEEN adjacent float32 coordinates.  Job 0 is the
    axis-aligned construction (centre 0.7 float32 steps past 5000 m, half width 1 m: the point one step past 5001 m is outside by 0.3 steps,
    and inside for a test that rounds the centre to float32); the others are rotated boxes with points within a few float32 steps of
    their faces.  One pair per box (both clouds the same frame and box)."""
    g = np.random.RandomState(seed)
    step = float(np.spacing(np.float32(5000.0)))
    boxes = [np.array([2.0, 1.0, 5000.0 + 0.7 * step, 2.0, 2.0, 4.0, 0.0])]
    q = [np.array([[2.0, 0.0, 5001.0 + k * step] for k in (-2, -1, 0, 1, 2, 3)] + [[2.0, 0.0, 4999.0 + k * step] for k in (-2, -1, 0, 1, 2, 3)])]
    for ry in (0.3, -1.1, 2.5, np.pi / 2, -2.0 * np.pi + 0.4, 0.0):
        b = draw_box(g)
        b[0] += -3000.0 + g.uniform(0, 1)
        b[2] += 4000.0 + g.uniform(0, 1)
        b[6] = ry
        # every point of a horizontal face shares ONE float32 height: keep both faces a good part of a float32 step away from it (and the
        # upper face away from height 0, where the float32 grid is finer than the undecided band)
        b[1] = float(np.float32(b[1] + 2.0)) + 0.3713 * float(np.spacing(np.float32(b[1] + 2.0)))
        b[3] = float(np.float32(b[3]))
        c, s = np.cos(ry), np.sin(ry)
        n = 160
        loc = np.stack([g.uniform(-1, 1, n) * b[5] / 2, -g.uniform(0, 1, n) * b[3], g.uniform(-1, 1, n) * b[4] / 2], 1)
        face = g.randint(0, 6, n)   # put every point on one of the six faces
        for k in range(n):
            a, sign = face[k] // 2, 1.0 if face[k] % 2 else -1.0
            loc[k, a] = (sign * b[5] / 2, -b[3] if sign > 0 else 0.0, sign * b[4] / 2)[a]
        cam = np.stack([c * loc[:, 0] + s * loc[:, 2], loc[:, 1], -s * loc[:, 0] + c * loc[:, 2]], 1) + b[:3]
        q.append(cam)
        boxes.append(b)
    pts = []
    for cam in q:
        p = to_velodyne(cam)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    m = p.copy()
                    for a, d in enumerate((dx, dy, dz)):
                        for _ in range(abs(d)):
                            m[:, a] = np.nextafter(m[:, a], np.float32(np.inf if d > 0 else -np.inf))
                    pts.append(m)
    scan = np.concatenate(pts, 0)
    boxes = np.array(boxes)
    return dict(scans=[pad_stride(scan, stride, g)], frames=np.zeros((len(boxes), 2), np.int32), boxes=np.stack([boxes, boxes], 1),
                dz=np.zeros((len(boxes), 2), np.float32))


def write_kitti_tree(root, seed=3, n_seq=2, n_frames=4, max_points=3000):
    """A tiny KITTI-shaped tree: training/velodyne/%04d/%06d.bin and training/label_02/%04d.txt.  Per sequence three tracks (a Car over all
    frames, a Pedestrian that is missing in frame 1, a Car that is DontCare-d / too occluded in places) moving a little from frame to frame."""
    import os
    g = np.random.RandomState(seed)
    for seq in range(n_seq):
        os.makedirs(os.path.join(root, "training", "velodyne", "%04d" % seq), exist_ok=True)
        os.makedirs(os.path.join(root, "training", "label_02"), exist_ok=True)
        tracks = [("Car", draw_box(g)), ("Pedestrian", draw_box(g)), ("Car", draw_box(g))]
        tracks[1][1][3:6] = [1.7, 0.6, 0.8]
        lines = []
        for f in range(n_frames):
            pts = [to_velodyne(g.uniform(-60, 60, (max_points // 4, 3)))]
            for t, (cls, b) in enumerate(tracks):
                b[:3] += g.uniform(-0.4, 0.4, 3)
                b[6] += g.uniform(-0.1, 0.1)
                if t == 1 and f == 1:
                    continue
                occl = 4 if (t == 2 and f == 2) else int(g.randint(0, 3))
                pts.append(points_around(g, b, max_points // 4, half=1.5))
                lines.append("%d %d %s %d %d %.6f %.2f %.2f %.2f %.2f %.6f %.6f %.6f %.6f %.6f %.6f %.6f" %
                             ((f, t, cls, int(g.randint(0, 3)), occl, g.uniform(-3, 3)) + tuple(g.uniform(0, 1200, 4)) +
                              (b[3], b[4], b[5], b[0], b[1], b[2], b[6])))
            lines.append("%d -1 DontCare -1 -1 -10.000000 10.00 20.00 30.00 40.00 -1000.000000 -1000.000000 -1000.000000 -10.000000 -1.000000 -1.000000 -1.000000" % f)
            scan = np.concatenate(pts, 0)
            scan = scan[g.permutation(len(scan))]
            pad_stride(scan, 4, g).tofile(os.path.join(root, "training", "velodyne", "%04d" % seq, "%06d.bin" % f))
        with open(os.path.join(root, "training", "label_02", "%04d.txt" % seq), "w") as fh:
            fh.write("\n".join(lines) + "\n")
