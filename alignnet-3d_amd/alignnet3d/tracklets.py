"""KITTI tracking labels and scans -> pairs of object clouds with labels (the KITTITracklets* datasets), host side.

The reference makes these datasets with FromKITTIScene (tp_utils/pointcloud.py:1000-1033): extract_pointcloud (:840-869) crops a Velodyne
scan to the tracked 3D box (compute_box_3d :918-940, extract_pc_in_box3d / in_hull :769-778), get_relative_transform (:888-906) and
get_transform_components (:876-885) give the labels, KittiTrackingLabels (:597-652) reads the label files.  Here the crop runs on the GPU
(csrc/alignnet_crop.hip, defined by tests/tracklet_ref.py) and this module restates the host side: label parsing, the pairing, the twelve
label columns, the meta record and the 4 x 4 transform.

extract_pointcloud's other branch, from_bbox2d (extract_pc_in_box2d :794-801 -> get_lidar_in_image_fov :781-791 ->
Calibration.project_velo_to_image :41-202), keeps every return whose image projection falls inside the label's 2D box: the crop a tracker
has before any 3D box exists.  extract(..., from_bbox2d=True, calib=..., image_size=...) runs it on the GPU (defined by
tests/frustum_ref.py); read_calib parses a calibration file as Calibration.read_calib_file does, projection multiplies P, R0 and V2C once,
read_image_size reads (W, H) from a PNG's header (all the reference takes from the image on this path).

What is this project's own: the reference's script that chooses WHICH (frame, frame) pairs of a track become examples is unpublished, the
selection of the `Hard` variants included; `pairs` therefore pairs one track id in frames f and f + gap, and `gap` and `min_points` are
options of this project, not the reference's.  No colour columns are produced (the reference reads [:, :3] everywhere, and colours need the
camera images' pixels).

Held data -- a tracker's own output, no ground truth -- is FromHeldScene's (:1036-1052): the two crops as they are, zero labels, and the meta keys
`trackid`, `frames`, `timestamps` that evaluation.evaluate_held turns into a speed per track.  held_pairs / held_meta / extract(..., held=True) make
it from label files in the same 17-column format (what trackers emit) and a timestamp per frame."""
import os
import struct
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


HeldPair = namedtuple("HeldPair", Pair._fields + ("timestamps",))


def read_timestamps(path):
    """A timestamp file: one value in seconds per frame, line f = frame f.  Returns a float64 array."""
    with open(path) as fh:
        return np.array([float(line) for line in fh if line.strip()], np.float64)


def rate_timestamps(frame_rate=10.0):
    """frame -> frame / frame_rate seconds, for data without a timestamp file (KITTI's scanner turns at 10 Hz)."""
    if not frame_rate > 0:
        raise ValueError("frame_rate = %r: expected > 0" % (frame_rate,))
    return lambda frame: float(frame) / float(frame_rate)


def held_pairs(labels, classes, timestamps, seq, gap=1, min_points=0, counts=None):
    """The pairs of pairs(...) as HeldPair: the same fields plus timestamps = (seconds of frame f, seconds of frame f + gap).  timestamps: a sequence
    indexed by frame number (read_timestamps) or a callable frame -> seconds (rate_timestamps).  As in pairs, no pair is made across a hole in a track."""
    at = timestamps if callable(timestamps) else lambda f: float(timestamps[f])
    out = []
    for p in pairs(labels, classes, gap=gap, min_points=min_points, counts=counts, seq=seq):
        try:
            ts = (float(at(p.frames[0])), float(at(p.frames[1])))
        except IndexError:
            raise ValueError("sequence %d: no timestamp for frame %d or %d (%d given)" % (seq, p.frames[0], p.frames[1], len(timestamps))) from None
        out.append(HeldPair(*p, ts))
    return out


HELD_TRACKID_STRIDE = 10000


def held_meta(pair):
    """Scene.save_meta + FromHeldScene.additional_meta (:986-997, 1043-1052): the base keys with zero positions, angles and translation (there is no
    ground truth), then class, frames, timestamps, trackid, in that order.  trackid = seq * 10000 + the label file's track id: THIS PROJECT'S rule --
    the reference's ids come from an unpublished tracker dump; all evaluate_held asks of them is that one object keeps one id and two objects differ,
    which holds for up to 10000 tracks per sequence.  `class` is the label's (the reference writes 'Car' for every held track)."""
    zero = np_to_str(np.zeros(3))
    return {"start_position": zero, "start_angle": 0.0, "end_position": zero, "end_angle": 0.0, "translation": zero, "rel_angle": 0.0,
            "class": pair.cls, "frames": [int(pair.frames[0]), int(pair.frames[1])], "timestamps": [float(pair.timestamps[0]), float(pair.timestamps[1])],
            "trackid": int(pair.seq) * HELD_TRACKID_STRIDE + int(pair.track)}


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


def extract_args(pair_list, frame_index, held=False):
    """(frames [B, 2] int32, boxes [B, 2, 7] float64, dz [B, 2] float32, labels [B, 12] float32) of Engine.tracklet_extract /
    tracklet_install_dataset: frame_index maps a pair's frame numbers to positions in the uploaded scans; dz = (0, float32(z_difference)).
    held=True (FromHeldScene): dz and the twelve label columns are zeros -- there is no ground truth to take z_difference from."""
    B = len(pair_list)
    frames, boxes, dz, lab = np.zeros((B, 2), np.int32), np.zeros((B, 2, 7)), np.zeros((B, 2), np.float32), np.zeros((B, 12), np.float32)
    for i, p in enumerate(pair_list):
        frames[i] = frame_index[p.frames[0]], frame_index[p.frames[1]]
        boxes[i, 0], boxes[i, 1] = p.box1, p.box2
        if held:
            continue
        l12, zd = labels12(p.box1, p.box2)
        dz[i, 1] = np.float32(zd)
        lab[i] = l12
    return frames, boxes, dz, lab


Calib = namedtuple("Calib", "P R0 V2C")


def read_calib(path):
    """A KITTI calibration file as Calib(P [3, 4] from P2, R0 [3, 3], V2C [3, 4]) float64.  Calibration.read_calib_file's parsing (:99-122):
    `key value ...` per line, ':' stripped from the key, a line whose values are not all floats is skipped.  The tracking files' names
    (Tr_velo_cam, R_rect) and the detection files' (Tr_velo_to_cam, R0_rect) are both accepted."""
    data = {}
    with open(path) as fh:
        for line in fh:
            line = line.rstrip()
            if not line:
                continue
            key, _, value = line.partition(" ")
            try:
                data[key.replace(":", "")] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass

    def field(names, shape):
        for n in names:
            if n in data:
                if data[n].size != shape[0] * shape[1]:
                    raise ValueError("%s: %s has %d values, expected %d" % (path, n, data[n].size, shape[0] * shape[1]))
                return data[n].reshape(shape)
        raise ValueError("%s: no %s line" % (path, " / ".join(names)))

    return Calib(field(("P2",), (3, 4)), field(("R_rect", "R0_rect"), (3, 3)), field(("Tr_velo_cam", "Tr_velo_to_cam"), (3, 4)))


def projection(calib):
    """M [3, 4] = P R0' V2C' (R0, V2C padded to 4 x 4) of a Calib: Velodyne point to homogeneous pixel, the three products of
    project_velo_to_image (:157-202) multiplied once.  These bits are what the device receives."""
    R4, V4 = np.eye(4), np.eye(4)
    R4[:3, :3] = np.asarray(calib.R0, np.float64).reshape(3, 3)
    V4[:3, :4] = np.asarray(calib.V2C, np.float64).reshape(3, 4)
    return np.matmul(np.asarray(calib.P, np.float64).reshape(3, 4), np.matmul(R4, V4))


def read_image_size(path):
    """(W, H) of a PNG from its first 24 bytes (signature, IHDR length and tag, width, height): im.size of the reference (:854, :857)."""
    with open(path, "rb") as fh:
        head = fh.read(24)
    if len(head) < 24 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError("%s: not a PNG header" % path)
    return struct.unpack(">II", head[16:24])


def frustum_args(pair_list, frame_index, calib, image_size):
    """(rects [B, 2, 4] float64, proj [F, 3, 4], image [F, 2]) of Engine.tracklet_extract_frustum.  calib: a Calib, a matrix M [3, 4], or
    {frame number: either}; image_size: (W, H) or {frame number: (W, H)}."""
    rects = np.zeros((len(pair_list), 2, 4))
    for i, p in enumerate(pair_list):
        rects[i, 0], rects[i, 1] = p.bbox2d1, p.bbox2d2
    of = lambda table, f: table[f] if isinstance(table, dict) else table
    proj, image = np.zeros((len(frame_index), 3, 4)), np.zeros((len(frame_index), 2))
    for f, i in frame_index.items():
        c = of(calib, f)
        proj[i] = projection(c) if isinstance(c, Calib) else np.asarray(c, np.float64).reshape(3, 4)
        image[i] = of(image_size, f)
    return rects, proj, image


def extract(engine, scans, pair_list, install=False, from_bbox2d=False, calib=None, image_size=None, clip=2.0, held=False):
    """Crop `pair_list` (pairs of ONE sequence) on the GPU.  scans: {frame number: float32 [n, 3 or 4]} or a list indexed by frame number;
    the frames the pairs use are uploaded in one call.  Returns the offsets table [B + 1, 2]; the crops stay on the device --
    engine.tracklet_read() copies them out, install=True makes them the HBM-resident dataset with the pairs' labels (sample_batch,
    train_step_rows, register_rows, ... then work on them).  from_bbox2d=True: the image-frustum crop to the pairs' bbox2d1 / bbox2d2 in
    place of the 3D boxes (calib, image_size: see frustum_args; clip: the reference's clip_distance); labels and dz are the same.
    held=True: both crops as they are (no z_difference subtracted from the second) and zero labels, as FromHeldScene has them."""
    if from_bbox2d and (calib is None or image_size is None):
        raise ValueError("from_bbox2d=True needs calib and image_size")
    get = scans.__getitem__
    used = sorted({f for p in pair_list for f in p.frames})
    index = {f: i for i, f in enumerate(used)}
    if not used:
        engine.tracklet_upload_scans((np.zeros((0, 4), np.float32), np.zeros(1, np.int64)))
    else:
        engine.tracklet_upload_scans([get(f) for f in used])
    frames, boxes, dz, lab = extract_args(pair_list, index, held=held)
    if from_bbox2d:
        rects, proj, image = frustum_args(pair_list, index, calib, image_size)
        off = engine.tracklet_extract_frustum(frames, rects, proj, image, dz, clip)
    else:
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
