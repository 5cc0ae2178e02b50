#!/usr/bin/env python3
"""Golden vectors for the scene generator's host side (alignnet3d/scenes.py) from the REFERENCE implementation: run only where the
reference tree exists (the GPU box never sees it).  tp_utils/pointcloud.py imports with the stubs of make_golden.py (no TensorFlow,
quaternion, trimesh, ... needed for what is recorded here):

  ray_directions       every 997th row of the module-level sensor table, and its first and last rows
  scene draws          (row i of every array belongs to scenes[i] of the JSON) for 20 seeds x {SyntheticScene, SyntheticScene(allow_persons=True), SyntheticSceneCats} x both object sets, after
                       np.random.seed(seed): cat, mesh_id, mesh_scale, start / end position and angle, translation, rel_angle and the
                       three 4 x 4 transforms

Outputs (committed, data only): tests/golden/scene_vectors.npz + scene_vectors.json."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, stub_modules  # noqa: E402

SEEDS = list(range(20))
CATS = ["airplane", "bench", "chair", "guitar", "sofa"]
KINDS = ("cars", "carspersons", "cats")
FIELDS = ("start_position", "end_position", "translation", "transform_start", "transform_end", "rel_transform")


def main():
    stub_modules()
    sys.path.insert(0, os.path.join(REF, "tp_utils"))
    sys.path.insert(0, REF)
    import pointcloud as P
    rows = sorted(set(list(range(0, P.n, 997)) + [0, P.n - 1]))
    out = {"ray_rows": np.array(rows, np.int64), "ray_directions": P.ray_directions[rows]}
    meta = {"seeds": SEEDS, "cats": CATS, "kinds": list(KINDS), "fields": list(FIELDS), "scenes": []}
    scalars, fields = [], {f: [] for f in FIELDS}
    for kind in KINDS:
        for second in (False, True):
            for seed in SEEDS:
                np.random.seed(seed)
                if kind == "cats":
                    s = P.SyntheticSceneCats(seed, 1, CATS, second_object_set=second)
                else:
                    s = P.SyntheticScene(seed, 1, second_object_set=second, allow_persons=kind == "carspersons")
                t = s.transform
                meta["scenes"].append({"kind": kind, "second_object_set": second, "seed": seed, "cat": str(s.cat), "mesh_id": int(s.mesh_id)})
                scalars.append([s.mesh_scale, t.start_angle, t.end_angle, t.rel_angle, t.angle, t.velocity])
                for f in FIELDS:
                    fields[f].append(np.asarray(getattr(t, f), np.float64))
    out["scalars"] = np.array(scalars, np.float64)   # row i belongs to meta["scenes"][i]
    for f in FIELDS:
        out[f] = np.stack(fields[f])
    np.savez_compressed(os.path.join(HERE, "scene_vectors.npz"), **out)
    json.dump(meta, open(os.path.join(HERE, "scene_vectors.json"), "w"), indent=1, sort_keys=True)
    print("scene golden: %d ray rows, %d scenes" % (len(rows), len(meta["scenes"])))


if __name__ == "__main__":
    main()
