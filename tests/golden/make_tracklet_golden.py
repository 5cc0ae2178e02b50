#!/usr/bin/env python3
"""Golden vectors for the KITTI tracklet extraction (alignnet3d/tracklets.py, tests/tracklet_ref.py) from the REFERENCE implementation: run
only where the reference tree exists (the GPU box never sees it).  tp_utils/pointcloud.py imports with the stubs of make_golden.py:

  boxes [40, 7]        drawn boxes (x, y, z, h, w, l, ry), ry beyond +-pi included; corners [40, 8, 3] = compute_box_3d
  pairs                boxes1 / boxes2 [40, 7]: get_relative_transform -> rel_transform [40, 4, 4], translation [40, 3], rel_angle [40],
                       rotation_center [40, 3], z_difference [40]; get_transform_components of both -> position1 / position2 [40, 3],
                       angle1 / angle2 [40]
  membership           for each of the first 10 boxes 500 drawn float32 points (camera frame) around it: hull_points [10, 500, 3] and
                       hull_inside [10, 500] = in_hull(points, compute_box_3d(box)) (scipy's Delaunay.find_simplex)

Outputs (committed, data only): tests/golden/tracklet_vectors.npz + tracklet_vectors.json."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, stub_modules  # noqa: E402

N_BOXES, N_HULL, N_POINTS, SEED = 40, 10, 500, 20


def draw_boxes(g, n):
    b = np.empty((n, 7))
    b[:, 0] = g.uniform(-30, 30, n)
    b[:, 1] = g.uniform(0.5, 2.5, n)
    b[:, 2] = g.uniform(2, 70, n)
    b[:, 3] = g.uniform(1.2, 2.2, n)
    b[:, 4] = g.uniform(0.5, 2.0, n)
    b[:, 5] = g.uniform(0.6, 5.0, n)
    b[:, 6] = g.uniform(-1.5 * np.pi, 1.5 * np.pi, n)
    return b


def main():
    stub_modules()
    sys.path.insert(0, os.path.join(REF, "tp_utils"))
    sys.path.insert(0, REF)
    import pointcloud as P
    g = np.random.RandomState(SEED)
    boxes = draw_boxes(g, N_BOXES)
    boxes2 = boxes.copy()
    boxes2[:, :3] += g.uniform(-1.5, 1.5, (N_BOXES, 3))
    boxes2[:, 6] += g.uniform(-0.6, 0.6, N_BOXES)
    out = {"boxes": boxes, "boxes1": boxes, "boxes2": boxes2, "corners": np.stack([P.compute_box_3d(b) for b in boxes])}
    rel = [P.get_relative_transform(b1.copy(), b2.copy()) for b1, b2 in zip(boxes, boxes2)]
    out["rel_transform"] = np.stack([r[0] for r in rel])
    out["translation"] = np.stack([r[1] for r in rel])
    out["rel_angle"] = np.array([r[2] for r in rel])
    out["rotation_center"] = np.stack([r[3] for r in rel])
    out["z_difference"] = np.array([r[4] for r in rel])
    for k, bb in ((1, boxes), (2, boxes2)):
        comp = [P.get_transform_components(b.copy()) for b in bb]
        out["position%d" % k] = np.stack([c[0] for c in comp])
        out["angle%d" % k] = np.array([c[1] for c in comp])
    pts = np.empty((N_HULL, N_POINTS, 3), np.float32)
    inside = np.empty((N_HULL, N_POINTS), bool)
    for i in range(N_HULL):
        centre = boxes[i, :3] - [0, boxes[i, 3] / 2, 0]
        pts[i] = (centre + g.uniform(-3.0, 3.0, (N_POINTS, 3))).astype(np.float32)
        inside[i] = P.in_hull(pts[i], P.compute_box_3d(boxes[i]))
    out["hull_points"], out["hull_inside"] = pts, inside
    np.savez_compressed(os.path.join(HERE, "tracklet_vectors.npz"), **out)
    meta = {"seed": SEED, "boxes": N_BOXES, "hull_boxes": N_HULL, "hull_points": N_POINTS, "inside_per_box": [int(x) for x in inside.sum(1)],
            "columns": "x y z h w l ry"}
    json.dump(meta, open(os.path.join(HERE, "tracklet_vectors.json"), "w"), indent=1, sort_keys=True)
    print("tracklet golden: %d boxes, %d pairs, %d x %d hull points (%d inside)" % (N_BOXES, N_BOXES, N_HULL, N_POINTS, int(inside.sum())))


if __name__ == "__main__":
    main()
