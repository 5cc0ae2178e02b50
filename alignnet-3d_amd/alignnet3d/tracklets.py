"""KITTI tracking labels and scans -> pairs of object clouds with labels (the KITTITracklets* datasets), host side.

The reference makes these datasets with FromKITTIScene (tp_utils/pointcloud.py:1000-1033): extract_pointcloud (:840-869) crops a Velodyne
scan to the tracked 3D box (compute_box_3d :918-940, extract_pc_in_box3d / in_hull :769-778), get_relative_transform (:888-906) and
get_transform_components (:876-885) give the labels, KittiTrackingLabels (:597-652) reads the label files.  Here the crop runs on the GPU
(csrc/alignnet_crop.hip, defined by tests/tracklet_ref.py) and this module restates the host side: label parsing, the pairing, the twelve
label columns, the meta record and the 4 x 4 transform.

What is this project's own: the reference's script that chooses WHICH (frame, frame) pairs of a track become examples is unpublished, the
selection of the `Hard` variants included; `pairs` therefore pairs one track id in frames f and f + gap, and `gap` and `min_points` are
options of this project, not the reference's.  No colour columns are produced (the reference reads [:, :3] everywhere, and colours need the
camera images); from_bbox2d (the image-frustum crop) and FromHeldScene are not provided."""
import os
from collections import namedtuple

import numpy as np

from .scenes import np_to_str

# R = R1 R2 (pointcloud.py:844-846): camera = R velodyne = (-y, -z, x); velodyne = camera @ R = (cz, -cx, -cy)
R = np.array([[0., -1., 0.], [0., 0., -1.], [1., 0., 0.]])
CLASSES = "Car Van Truck Pedestrian Person_sitting Cyclist Tram Misc DontCare".split()
COLUMNS = 17   # frame id class truncated occluded alpha x1 y1 x2 y2 h w l x y z ry

Labels = namedtuple("Labels", "frame track cls truncated occluded alpha bbox2d box")
Pair = namedtuple("Pair", "seq frames track cls truncated occluded box1 box2 bbox2d1 bbox2d2 rows")


def read_labels(path, truncated_threshold=(0, 2), occluded_threshold=(0, 3)):
    """A KITTI tracking label file (label_02/%04d.txt, the 17 published columns) as Labels of arrays, one entry per kept row in file order:
    frame, track (the file's id), cls (str), truncated, occluded, alpha, bbox2d [n, 4] = x1 y1 x2 y2, box [n, 7] = (x, y, z, h, w, l, ry) float64.
    As KittiTrackingLabels does: the real-valued columns are rounded to float32 and widened again (:621-623), DontCare rows are dropped
    (:619), and only rows with 0 <= occluded <= 3 and 0 <= truncated <= 2 are kept (:606, :631-635)."""
    rows = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            tok = line.split()
            if not tok:
                continue
            if len(tok) < COLUMNS:
                raise ValueError("%s:%d: %d columns, expected %d" % (path, ln, len(tok), COLUMNS))
            rows.append(tok[:COLUMNS])
    f32 = lambda t: float(np.float32(float(t)))
    keep = []
    for t in rows:
        if t[2] == "DontCare":
            continue
        trunc, occ = f32(t[3]), f32(t[4])
        if not (occluded_threshold[0] <= occ <= occluded_threshold[1] and truncated_threshold[0] <= trunc <= truncated_threshold[1]):
            continue
        v = [f32(x) for x in t[5:17]]   # alpha x1 y1 x2 y2 h w l x y z ry
        keep.append((int(t[0]), int(t[1]), t[2], trunc, occ, v[0], v[1:5], [v[8], v[9], v[10], v[5], v[6], v[7], v[11]]))
    col = lambda i, dt: np.array([k[i] for k in keep], dt)
    return Labels(col(0, np.int64), col(1, np.int64), [k[2] for k in keep], col(3, np.float64), col(4, np.float64), col(5, np.float64),
                  np.array([k[6] for k in keep], np.float64).reshape(-1, 4), np.array([k[7] for k in keep], np.float64).reshape(-1, 7))


def pairs(labels, classes=("Car",), gap=1, min_points=0, counts=None, seq=0):
    """Pairs of one track id in frames f and f + gap, both rows of a class in `classes`, ordered by (first frame, track id).  A track that
    leaves and comes back makes no pair across the hole unless the two frames are exactly `gap` apart.  min_points > 0 keeps a pair only when
    both of its boxes hold at least that many scan points: counts [rows] then gives the points inside every label row's box (from a first
    extraction; filter_min_points does the same from an offsets table).  This pairing is this project's: the reference's is unpublished."""
    if gap < 1:
        raise ValueError("gap = %r: expected >= 1" % (gap,))
    if min_points > 0 and counts is None:
        raise ValueError("min_points > 0 needs counts (points per label row)")
    where = {(int(f), int(t)): i for i, (f, t) in enumerate(zip(labels.frame, labels.track))}
    out = []
    for (f, t), i in sorted(where.items()):
        j = where.get((f + gap, t))
        if j is None or labels.cls[i] not in classes or labels.cls[j] != labels.cls[i]:
            continue
        if min_points > 0 and (counts[i] < min_points or counts[j] < min_points):
            continue
        out.append(Pair(int(seq), (f, f + gap), t, labels.cls[i], float(labels.truncated[i]), float(labels.occluded[i]), labels.box[i].copy(),
                        labels.box[j].copy(), labels.bbox2d[i].copy(), labels.bbox2d[j].copy(), (i, j)))
    return out


def filter_min_points(pair_list, offsets, min_points):
    """The pairs whose two crops (offsets: the table of the extraction of pair_list) both hold at least min_points points, and their indices."""
    n = np.diff(np.asarray(offsets), axis=0)
    idx = [i for i in range(len(pair_list)) if n[i].min() >= min_points]
    return [pair_list[i] for i in idx], idx


def box_corners(box):
    """compute_box_3d (:918-940): the eight corners [8, 3] in the camera frame."""
    b = np.asarray(box, np.float64)
    c, s = np.cos(b[6]), np.sin(b[6])
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    h, w, l = b[3:6]
    x = [l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2]
    y = [0, 0, 0, 0, -h, -h, -h, -h]
    z = [w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2]
    return (np.dot(rot, np.vstack([x, y, z])) + b[:3, None]).T


def transform_components(box):
    """get_transform_components (:876-885): (position in the Velodyne frame, raised by h / 2; angle = ry)."""
    b = np.asarray(box, np.float64)
    position = np.matmul(b[:3], R)
    position[2] += b[3] / 2.0
    return position, float(b[6])


def mat_angle(translation, angle, center):
    """get_mat_angle (:279-289): rotation by `angle` about the z axis through `center`, then `translation`."""
    m1, m2, m3 = np.eye(4), np.eye(4), np.eye(4)
    m1[:3, 3] = -center
    m3[:3, 3] = center + translation
    c, s = np.cos(angle), np.sin(angle)
    m2[:2, :2] = [[c, -s], [s, c]]
    return np.matmul(np.matmul(m3, m2), m1)


def relative_transform(box1, box2):
    """get_relative_transform (:888-906): (rel_transform [4, 4], translation [3] with z zeroed, rel_angle -- NOT wrapped to +-pi: the
    reference leaves it (:896) --, rotation_center [3], z_difference), all in the Velodyne frame."""
    b1, b2 = np.asarray(box1, np.float64), np.asarray(box2, np.float64)
    translation = np.matmul(b2[:3] - b1[:3], R)
    angle = float(b2[6] - b1[6])
    z_difference = float(translation[2])
    translation[2] = 0.0
    center = np.matmul(b1[:3], R)
    return mat_angle(translation, angle, center), translation, angle, center, z_difference


def labels12(box1, box2):
    """(the 12 label columns of alignnet3d/packed.py float64 -- translation, rel_angle, start_position, end_position, start_angle, end_angle
    as FromKITTIScene sets them (:1013-1020) --, z_difference)."""
    _, translation, angle, _, zd = relative_transform(box1, box2)
    p1, a1 = transform_components(box1)
    p2, a2 = transform_components(box2)
    return np.concatenate([translation, [angle], p1, p2, [a1, a2]]), zd


def vo_matrix(vo):
    """R4^T vo R4 (:848-851): a visual-odometry pose of the camera frame in the Velodyne frame."""
    R4 = np.eye(4)
    R4[:3, :3] = R
    return np.matmul(R4.T, np.matmul(np.asarray(vo, np.float64).reshape(4, 4), R4))


def meta(pair, vo1=None, vo2=None):
    """Scene.save_meta + FromKITTIScene.additional_meta (:986-997, 1022-1033): the same keys in the same order.  vo1 / vo2: the 4 x 4
    visual-odometry matrices as read from the pose files (float32 text), None = the identity."""
    lab, _ = labels12(pair.box1, pair.box2)
    vo = [np.eye(4) if v is None else vo_matrix(np.asarray(v, np.float32)) for v in (vo1, vo2)]
    return {"start_position": np_to_str(lab[4:7]), "start_angle": float(lab[10]), "end_position": np_to_str(lab[7:10]), "end_angle": float(lab[11]),
            "translation": np_to_str(lab[0:3]), "rel_angle": float(lab[3]),
            "class": pair.cls, "truncated": pair.truncated, "occluded": pair.occluded, "seq": pair.seq, "frames": [int(pair.frames[0]), int(pair.frames[1])],
            "trackids": [int(pair.track), int(pair.track)], "vo1": np_to_str(vo[0]), "vo2": np_to_str(vo[1]),
            "bbox3ds": [np_to_str(pair.box1), np_to_str(pair.box2)], "bbox2ds": [np_to_str(pair.bbox2d1), np_to_str(pair.bbox2d2)]}


def extract_args(pair_list, frame_index):
    """(frames [B, 2] int32, boxes [B, 2, 7] float64, dz [B, 2] float32, labels [B, 12] float32) of Engine.tracklet_extract /
    tracklet_install_dataset: frame_index maps a pair's frame numbers to positions in the uploaded scans; dz = (0, float32(z_difference))."""
    B = len(pair_list)
    frames, boxes, dz, lab = np.zeros((B, 2), np.int32), np.zeros((B, 2, 7)), np.zeros((B, 2), np.float32), np.zeros((B, 12), np.float32)
    for i, p in enumerate(pair_list):
        frames[i] = frame_index[p.frames[0]], frame_index[p.frames[1]]
        boxes[i, 0], boxes[i, 1] = p.box1, p.box2
        l12, zd = labels12(p.box1, p.box2)
        dz[i, 1] = np.float32(zd)
        lab[i] = l12
    return frames, boxes, dz, lab


def extract(engine, scans, pair_list, install=False):
    """Crop `pair_list` (pairs of ONE sequence) on the GPU.  scans: {frame number: float32 [n, 3 or 4]} or a list indexed by frame number;
    the frames the pairs use are uploaded in one call.  Returns the offsets table [B + 1, 2]; the crops stay on the device --
    engine.tracklet_read() copies them out, install=True makes them the HBM-resident dataset with the pairs' labels (sample_batch,
    train_step_rows, register_rows, ... then work on them)."""
    get = scans.__getitem__
    used = sorted({f for p in pair_list for f in p.frames})
    index = {f: i for i, f in enumerate(used)}
    if not used:
        engine.tracklet_upload_scans((np.zeros((0, 4), np.float32), np.zeros(1, np.int64)))
    else:
        engine.tracklet_upload_scans([get(f) for f in used])
    frames, boxes, dz, lab = extract_args(pair_list, index)
    off = engine.tracklet_extract(frames, boxes, dz)
    if install:
        engine.tracklet_install_dataset(lab)
    return off


def read_scan(root, seq, frame):
    """training/velodyne/%04d/%06d.bin: float32 [n, 4]."""
    return np.fromfile(os.path.join(root, "training", "velodyne", "%04d" % seq, "%06d.bin" % frame), dtype=np.float32).reshape(-1, 4)


def read_vo(vo_dir, seq, frame):
    """vo_%04d_%06d.txt (:848), float32 text; None when the directory or the file is missing."""
    if not vo_dir:
        return None
    path = os.path.join(vo_dir, "vo_%04d_%06d.txt" % (seq, frame))
    return np.loadtxt(path, dtype=np.float32).reshape(4, 4) if os.path.isfile(path) else None
