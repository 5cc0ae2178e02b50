#!/usr/bin/env python3
"""Tracks to trajectories: multiway registration of a tracker's crops (Engine.pose_graph_optimize; alignnet3d/tracks.py).

    python track_graph.py --config F --model CKPT --kitti DIR --out OUT --max-skip K [--from-bbox2d] [--refine p2p|plane|generalized] [--threshold T]

DIR is a tracker's label tree as make_kitti_dataset.py --held reads it (training/velodyne/%04d/%06d.bin, training/label_02/%04d.txt in the 17-column
format; timestamps from --timestamps-dir/%04d.txt or --frame-rate).  Per sequence: the pairs of every track at gaps 1 .. K (tracklets.held_pairs), their
crops on the device as the resident dataset (tracklets.extract), ONE register_rows call (the network, and ICP on the full crops with --refine), ONE
evaluate_registration_rows call for the information matrices about the target crops' means.  Then every unbroken stretch of a track becomes a pose graph
(a node per frame, a certain edge per gap-1 pair, an uncertain edge per longer pair) and ONE pose_graph_optimize call solves them all.
Written per graph: OUT/track<trackid>.json (frames, timestamps, chained poses, optimised poses, edges with weights and the pruned ones, objective) and
OUT/track<trackid>.txt (the xy speed of the object between consecutive optimised poses, one value per line: tracks.speeds).  trackid is
make_kitti_dataset.py's (sequence * 10000 + track id); a later stretch of a track that a hole has split is written as track<trackid>_<first frame>.
evaluation.evaluate_held and its files are not touched: this is another consumer of the same tracker output."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

REFINE = {None: None, "p2p": "point", "plane": "plane", "generalized": "generalized"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="Config file of the model")
    ap.add_argument("--model", required=True, help="Checkpoint (.aln3)")
    ap.add_argument("--kitti", required=True, help="tracker output (training/velodyne/%%04d/%%06d.bin, training/label_02/%%04d.txt)")
    ap.add_argument("--out", required=True, help="directory to write track<trackid>.json / .txt into")
    ap.add_argument("--max-skip", type=int, required=True, help="pairs of a track's frames f and f + s for s = 1 .. K become edges")
    ap.add_argument("--classes", default="Car", help="comma-separated KITTI classes")
    ap.add_argument("--from-bbox2d", action="store_true", help="crop to the image frustum of the label's 2D box instead of the 3D box")
    ap.add_argument("--calib-dir", default=None, help="with --from-bbox2d: directory of %%04d.txt calibration files (default <kitti>/training/calib)")
    ap.add_argument("--image-dir", default=None, help="with --from-bbox2d: directory of %%04d/%%06d.png, read for their size only")
    ap.add_argument("--image-size", default=None, metavar="W,H", help="with --from-bbox2d: the image size of every frame; no image is read")
    ap.add_argument("--clip", type=float, default=2.0, help="with --from-bbox2d: keep points with x > clip")
    ap.add_argument("--timestamps-dir", default=None, help="directory of %%04d.txt, one timestamp in seconds per frame")
    ap.add_argument("--frame-rate", type=float, default=10.0, help="without --timestamps-dir: t = frame / rate")
    ap.add_argument("--refine", choices=["p2p", "plane", "generalized"], default=None, help="ICP refinement of the network's transforms on the full crops")
    ap.add_argument("--its", type=int, default=30, help="ICP iterations")
    ap.add_argument("--threshold", type=float, default=0.02, help="inlier distance of the information matrices, and of the line process's mu")
    ap.add_argument("--preference", type=float, default=1.0, help="Open3D's preference_loop_closure")
    ap.add_argument("--full-rotation", action="store_true", help="six unknowns per pose instead of yaw + translation")
    ap.add_argument("--seed", type=int, default=0, help="Seed of the sampler's draw")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    args.classes = [c for c in args.classes.split(",") if c]
    if args.max_skip < 1:
        ap.error("--max-skip must be >= 1")
    if not args.threshold > 0:
        ap.error("--threshold must be > 0")
    if args.image_size is not None:
        try:
            w, h = (float(s) for s in args.image_size.split(","))
        except ValueError:
            ap.error("--image-size: W,H")
        args.image_size = (w, h)
    args.calib_dir = args.calib_dir or os.path.join(args.kitti, "training", "calib")
    args.image_dir = args.image_dir or os.path.join(args.kitti, "training", "image_02")
    return args


def sequence_edges(eng, T, args, seq):
    """(pairs, transforms, informations, centres, anchors) of one sequence; anchors [B, 3]: the mean of each pair's FIRST crop."""
    labels = T.read_labels(os.path.join(args.kitti, "training", "label_02", "%04d.txt" % seq))
    stamps = T.read_timestamps(os.path.join(args.timestamps_dir, "%04d.txt" % seq)) if args.timestamps_dir else T.rate_timestamps(args.frame_rate)
    pairs = [p for s in range(1, args.max_skip + 1) for p in T.held_pairs(labels, args.classes, stamps, seq, gap=s)]
    if not pairs:
        return None
    scans = {f: T.read_scan(args.kitti, seq, f) for f in sorted({f for p in pairs for f in p.frames})}
    if args.from_bbox2d:
        calib = T.read_calib(os.path.join(args.calib_dir, "%04d.txt" % seq))
        size = args.image_size or {f: T.read_image_size(os.path.join(args.image_dir, "%04d" % seq, "%06d.png" % f)) for f in scans}
        off = T.extract(eng, scans, pairs, install=True, from_bbox2d=True, calib=calib, image_size=size, clip=args.clip, held=True)
    else:
        off = T.extract(eng, scans, pairs, install=True, held=True)
    p1, p2 = eng.tracklet_read(off)
    mean = lambda p, lo, hi: p[lo:hi].astype(np.float64).mean(0) if hi > lo else np.zeros(3)
    anchors = np.stack([mean(p1, off[b, 0], off[b + 1, 0]) for b in range(len(pairs))])
    centres = np.stack([mean(p2, off[b, 1], off[b + 1, 1]) for b in range(len(pairs))])
    rows = np.arange(len(pairs), dtype=np.int32)
    reg = eng.register_rows(rows, args.seed, refine=REFINE[args.refine], its=args.its)
    ev = eng.evaluate_registration_rows(rows, reg["transforms"], threshold=args.threshold, centers=centres, want_information=True)
    return pairs, reg["transforms"], ev["information"], centres, anchors


def track_name(T, g):
    name = "track%d" % (g["seq"] * T.HELD_TRACKID_STRIDE + g["track"])
    return name if g["first"] else "%s_%d" % (name, int(g["frames"][0]))


def write_track(out_dir, name, g, res, anchor):
    from alignnet3d import tracks
    rec = {"seq": g["seq"], "track": g["track"], "frames": [int(f) for f in g["frames"]], "timestamps": [float(t) for t in g["timestamps"]],
           "anchor": [float(v) for v in anchor], "chained_poses": g["poses"].tolist(), "poses": res["poses"].tolist(),
           "objective": [res["before"], res["after"]], "solves": res["solves"], "status": res["status"], "mu": res["mu"],
           "edges": [{"frames": [int(g["frames"][i]), int(g["frames"][j])], "uncertain": bool(u), "transform": Tm.tolist(), "information": L.tolist(),
                      "centre": c.tolist(), "chi2": float(x), "weight": float(w), "pruned": bool(p)}
                     for i, j, u, Tm, L, c, x, w, p in zip(g["i"], g["j"], g["uncertain"], g["T"], g["info"], g["c"], res["chi2"], res["weights"], res["pruned"])],
           "pruned": [[int(g["frames"][i]), int(g["frames"][j])] for i, j, p in zip(g["i"], g["j"], res["pruned"]) if p]}
    with open(os.path.join(out_dir, name + ".json"), "w") as fh:
        json.dump(rec, fh)
    with open(os.path.join(out_dir, name + ".txt"), "w") as fh:
        fh.write("".join("%s\n" % repr(float(v)) for v in tracks.speeds(res["poses"], g["timestamps"], anchor)))


def main(argv=None):
    args = parse_args(argv)
    from config import load_config, configGlobal as cfg
    load_config(args.config)
    import alignnet3d
    from alignnet3d import tracklets as T, tracks
    from make_kitti_dataset import sequences
    eng = alignnet3d.Engine(cfg, device=args.device)
    eng.load(args.model)
    t0 = time.perf_counter()
    graphs, anchors = [], []
    for seq in sequences(args.kitti):
        got = sequence_edges(eng, T, args, seq)
        if got is None:
            continue
        pairs, transforms, informations, centres, first_means = got
        seen = set()
        for g in tracks.build_graphs(pairs, transforms, informations, centres, args.max_skip):
            g["first"] = (g["seq"], g["track"]) not in seen
            seen.add((g["seq"], g["track"]))
            graphs.append(g)
            # the object in the stretch's first frame: the first crop of a pair that starts there
            anchors.append(first_means[[b for b in g["pair_index"] if pairs[b].frames[0] == g["frames"][0]][0]] if len(g["pair_index"]) else np.zeros(3))
    results = eng.pose_graph_optimize(graphs, constrained=not args.full_rotation, preference=args.preference, threshold=args.threshold)
    eng.close()
    os.makedirs(args.out, exist_ok=True)
    for g, res, anchor in zip(graphs, results, anchors):
        write_track(args.out, track_name(T, g), g, res, anchor)
    pruned = sum(int(r["pruned"].sum()) for r in results)
    print("Track graphs: %d graphs, %d edges (%d pruned), max skip %d, %.2f s -> %s" %
          (len(graphs), sum(len(g["i"]) for g in graphs), pruned, args.max_skip, time.perf_counter() - t0, args.out))
    return graphs, results


if __name__ == "__main__":
    main()
