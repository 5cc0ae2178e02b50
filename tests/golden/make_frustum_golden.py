#!/usr/bin/env python3
"""Golden vectors for the image-frustum crop (alignnet3d/tracklets.py, tests/frustum_ref.py) from the REFERENCE implementation: run only
where the reference tree exists (the GPU box never sees it).  tp_utils/pointcloud.py imports with the stubs of make_golden.py:

  calibration          a tracking-format calibration file written here (tests/frustum_cases.KITTI: the numbers are data) parsed by the
                       reference's Calibration: P [3, 4], R0 [3, 3], V2C [3, 4]
  points [2000, 3]     float32 Velodyne points in front of and behind the sensor, inside and outside the image
  uv [2000, 2]         Calibration.project_velo_to_image(points)
  fov [2000]           get_lidar_in_image_fov(points, calib, 0, 0, W, H, return_more=True)'s mask (clip distance 2.0)
  rects [8, 4]         drawn rectangles, some beyond the image; members [8, 2000] = the rows extract_pc_in_box2d keeps, with an index column
                       as `pc`

Outputs (committed, data only): tests/golden/frustum_vectors.npz + frustum_vectors.json."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "alignnet-3d_amd"))
from make_golden import REF, stub_modules  # noqa: E402

N_POINTS, N_RECTS, SEED = 2000, 8, 31


def main():
    from tests import frustum_cases as C
    stub_modules()
    sys.path.insert(0, os.path.join(REF, "tp_utils"))
    sys.path.insert(0, REF)
    import pointcloud as P
    g = np.random.RandomState(SEED)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "0000.txt")
        with open(path, "w") as fh:
            fh.write(C.calib_text(C.KITTI, "tracking"))
        calib = P.Calibration(path)
    W, H = (int(v) for v in C.KITTI_IMAGE)
    x = np.concatenate([g.uniform(2.5, 60, N_POINTS - 600), g.uniform(-40, 2.5, 600)])
    pts = np.stack([x, -np.abs(x) * g.uniform(-1.3, 1.3, N_POINTS), -np.abs(x) * g.uniform(-0.45, 0.45, N_POINTS)], 1).astype(np.float32)
    pts = pts[g.permutation(N_POINTS)]
    uv = calib.project_velo_to_image(pts)
    _, uv2, fov = P.get_lidar_in_image_fov(pts, calib, 0, 0, W, H, True)
    assert np.array_equal(uv, uv2, equal_nan=True)
    rects = np.empty((N_RECTS, 4))
    rects[:, 0], rects[:, 1] = g.uniform(-100, W - 100, N_RECTS), g.uniform(-50, H - 80, N_RECTS)
    rects[:, 2], rects[:, 3] = rects[:, 0] + g.uniform(80, 500, N_RECTS), rects[:, 1] + g.uniform(60, 250, N_RECTS)
    rects[0], rects[1] = [W - 200, 100, W + 150, 300], [-80, -40, 250, H + 30]   # beyond the image on every side between them
    index = np.arange(N_POINTS).reshape(-1, 1)
    members = np.zeros((N_RECTS, N_POINTS), bool)
    for i, r in enumerate(rects):
        members[i, P.extract_pc_in_box2d(index, pts, r, calib, W, H)[:, 0]] = True
    out = {"P": calib.P, "R0": calib.R0, "V2C": calib.V2C, "image": np.array([W, H]), "points": pts, "uv": uv, "fov": fov, "rects": rects,
           "members": members}
    np.savez_compressed(os.path.join(HERE, "frustum_vectors.npz"), **out)
    meta = {"seed": SEED, "points": N_POINTS, "rects": N_RECTS, "in_image_and_front": int(fov.sum()), "members_per_rect": [int(m) for m in members.sum(1)],
            "clip_distance": 2.0, "rect_columns": "xmin ymin xmax ymax"}
    json.dump(meta, open(os.path.join(HERE, "frustum_vectors.json"), "w"), indent=1, sort_keys=True)
    print("frustum golden: %d points (%d in the image and in front), %d rectangles holding %s" % (N_POINTS, int(fov.sum()), N_RECTS, meta["members_per_rect"]))


if __name__ == "__main__":
    main()
