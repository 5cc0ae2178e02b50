#!/usr/bin/env python3
"""Make a KITTITracklets-style dataset from KITTI tracking data on the GPU, in the reference's on-disk layout.

The reference's KITTITrackletsCars / KITTITrackletsCarsPersons datasets come from FromKITTIScene (tp_utils/pointcloud.py:1000-1033): a
Velodyne scan is cropped to a tracked 3D box (scipy's Delaunay on the box's corners) in two frames of one track.  Here the labels are read
and paired by alignnet3d/tracklets.py and the crops are made by the engine (csrc/alignnet_crop.hip): the same points, in scan order.

    python make_kitti_dataset.py --kitti /data/kitti_tracking --out data/KITTITrackletsCars --classes Car
    python make_kitti_dataset.py --kitti /data/kitti_tracking --out data/KITTITrackletsCarsPersons --classes Car,Pedestrian --gap 2

--kitti ROOT holds training/velodyne/%04d/%06d.bin and training/label_02/%04d.txt.  Written: meta/%08d.json (the keys of Scene.save_meta +
FromKITTIScene), pointcloud{1,2}/%08d.npy (float64 [n, 3]), transform/%08d.npy (rel_transform), split/train.txt, split/val.txt.  train.py,
evaluation.py, icp_global.py and icp_global_fast.py run on it as it is.
Which frame pairs the reference used is unpublished (its pairing script is not part of the release, the selection of the `Hard` variants
included): --gap (a track's frames f and f + gap form a pair) and --min-points (both crops hold at least that many points) are this
project's options.  --val-seqs lists the sequences whose pairs go to split/val.txt.  --vo-dir DIR reads vo_%04d_%06d.txt pose files for the
meta's vo1 / vo2 (the identity without it).  One sequence's frames are uploaded per engine call.  No colour columns are written.
--from-bbox2d takes the reference's other crop (extract_pointcloud's from_bbox2d branch): every return whose image projection falls inside
the label's 2D box, the object together with ground and background.  It reads --calib-dir/%04d.txt (default ROOT/training/calib) and, for
each frame's image size, the header of --image-dir/%04d/%06d.png (default ROOT/training/image_02) unless --image-size W,H gives it;
--clip is the reference's clip_distance (2.0).  Meta, labels, transform and split files are the same as without it.
--held makes a HELD dataset (FromHeldScene, tp_utils/pointcloud.py:1036-1052) from a tracker's own output: label files in the same 17-column
format (further columns are ignored), no ground truth.  Both crops are written as they are, the labels are zeros, transform/ is the identity,
the meta carries trackid (sequence * 10000 + track id), frames and timestamps, and every pair goes to split/val.txt.  The timestamps come from
--timestamps-dir/%04d.txt (one value in seconds per frame) or from --frame-rate (t = frame / rate, default 10).  train.py evaluates such a set
with evaluation.special.mode = "held" (evaluation.evaluate_held: a smoothed speed per track).

    python make_kitti_dataset.py --kitti /data/my_tracker --out data/Held --held --from-bbox2d --frame-rate 10"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--kitti", required=True, help="KITTI tracking root (training/velodyne/%%04d/%%06d.bin, training/label_02/%%04d.txt)")
    ap.add_argument("--out", required=True, help="dataset directory to write")
    ap.add_argument("--classes", default="Car", help="comma-separated KITTI classes, e.g. Car or Car,Pedestrian")
    ap.add_argument("--gap", type=int, default=1, help="a track's frames f and f + gap form a pair")
    ap.add_argument("--min-points", type=int, default=1, help="keep a pair only when both crops hold at least this many points")
    ap.add_argument("--val-seqs", default="", help="comma-separated sequence numbers whose pairs form split/val.txt")
    ap.add_argument("--vo-dir", default=None, help="directory of vo_%%04d_%%06d.txt visual-odometry poses (meta vo1 / vo2)")
    ap.add_argument("--from-bbox2d", action="store_true", help="crop to the image frustum of the label's 2D box instead of the 3D box")
    ap.add_argument("--calib-dir", default=None, help="with --from-bbox2d: directory of %%04d.txt calibration files (default <kitti>/training/calib)")
    ap.add_argument("--image-dir", default=None, help="with --from-bbox2d: directory of %%04d/%%06d.png, read for their size only (default <kitti>/training/image_02)")
    ap.add_argument("--image-size", default=None, metavar="W,H", help="with --from-bbox2d: the image size of every frame; no image is read")
    ap.add_argument("--clip", type=float, default=2.0, help="with --from-bbox2d: keep points with x > clip (the reference's clip_distance)")
    ap.add_argument("--held", action="store_true", help="held data (a tracker's output, no ground truth): zero labels, trackid / timestamps in the meta, all pairs in val")
    ap.add_argument("--timestamps-dir", default=None, help="with --held: directory of %%04d.txt, one timestamp in seconds per frame")
    ap.add_argument("--frame-rate", type=float, default=10.0, help="with --held and no --timestamps-dir: t = frame / rate")
    ap.add_argument("--device", type=int, default=0)
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    args.classes = [c for c in args.classes.split(",") if c]
    if not args.classes:
        ap.error("--classes: at least one class")
    if args.gap < 1:
        ap.error("--gap must be >= 1")
    if args.min_points < 0:
        ap.error("--min-points must be >= 0")
    try:
        args.val_seqs = sorted({int(s) for s in args.val_seqs.split(",") if s})
    except ValueError:
        ap.error("--val-seqs: comma-separated integers")
    if args.image_size is not None:
        try:
            w, h = (float(s) for s in args.image_size.split(","))
        except ValueError:
            ap.error("--image-size: W,H")
        if not (w > 0 and h > 0):
            ap.error("--image-size: W and H must be > 0")
        args.image_size = (w, h)
    if not np.isfinite(args.clip):
        ap.error("--clip must be finite")
    if not (np.isfinite(args.frame_rate) and args.frame_rate > 0):
        ap.error("--frame-rate must be > 0")
    args.calib_dir = args.calib_dir or os.path.join(args.kitti, "training", "calib")
    args.image_dir = args.image_dir or os.path.join(args.kitti, "training", "image_02")
    return args


def sequences(root):
    d = os.path.join(root, "training", "label_02")
    return sorted(int(n[:-4]) for n in os.listdir(d) if n.endswith(".txt") and n[:-4].isdigit())


def write_example(T, root, index, pair, pc1, pc2, vo_dir=None):
    stem = str(index).zfill(8)
    for sub in ("meta", "pointcloud1", "pointcloud2", "transform", "split"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    held = hasattr(pair, "timestamps")
    with open(os.path.join(root, "meta", stem + ".json"), "w") as fh:
        json.dump(T.held_meta(pair) if held else T.meta(pair, T.read_vo(vo_dir, pair.seq, pair.frames[0]), T.read_vo(vo_dir, pair.seq, pair.frames[1])), fh)
    np.save(os.path.join(root, "pointcloud1", stem), np.asarray(pc1, np.float64))
    np.save(os.path.join(root, "pointcloud2", stem), np.asarray(pc2, np.float64))
    np.save(os.path.join(root, "transform", stem), np.eye(4) if held else T.relative_transform(pair.box1, pair.box2)[0])


def main(argv=None):
    args = parse_args(argv)
    import alignnet3d
    from alignnet3d import tracklets as T
    eng = alignnet3d.Engine(device=args.device)
    t0 = time.perf_counter()
    split = {"train": [], "val": []}
    n = points = 0
    for seq in sequences(args.kitti):
        labels = T.read_labels(os.path.join(args.kitti, "training", "label_02", "%04d.txt" % seq))
        if args.held:
            stamps = T.read_timestamps(os.path.join(args.timestamps_dir, "%04d.txt" % seq)) if args.timestamps_dir else T.rate_timestamps(args.frame_rate)
            cand = T.held_pairs(labels, args.classes, stamps, seq, gap=args.gap)
        else:
            cand = T.pairs(labels, args.classes, gap=args.gap, seq=seq)
        if not cand:
            continue
        scans = {f: T.read_scan(args.kitti, seq, f) for f in sorted({f for p in cand for f in p.frames})}
        if args.from_bbox2d:
            calib = T.read_calib(os.path.join(args.calib_dir, "%04d.txt" % seq))
            size = args.image_size or {f: T.read_image_size(os.path.join(args.image_dir, "%04d" % seq, "%06d.png" % f)) for f in scans}
            off = T.extract(eng, scans, cand, from_bbox2d=True, calib=calib, image_size=size, clip=args.clip, held=args.held)
        else:
            off = T.extract(eng, scans, cand, held=args.held)
        p1, p2 = eng.tracklet_read(off)
        kept, idx = T.filter_min_points(cand, off, args.min_points)
        for pair, i in zip(kept, idx):
            write_example(T, args.out, n, pair, p1[off[i, 0]:off[i + 1, 0]], p2[off[i, 1]:off[i + 1, 1]], args.vo_dir)
            split["val" if args.held or seq in args.val_seqs else "train"].append(n)   # (a held set has no train split)
            points += int(off[i + 1].sum() - off[i].sum())
            n += 1
    eng.close()
    os.makedirs(os.path.join(args.out, "split"), exist_ok=True)
    for name, ids in split.items():
        with open(os.path.join(args.out, "split", name + ".txt"), "w") as fh:
            fh.write("".join("%d\n" % i for i in ids))
    print("wrote %d pairs (%d train, %d val) to %s: %.1f points per cloud, classes %s, gap %d, %.2f s" %
          (n, len(split["train"]), len(split["val"]), args.out, points / (2.0 * max(n, 1)), ",".join(args.classes), args.gap, time.perf_counter() - t0))


if __name__ == "__main__":
    main()
