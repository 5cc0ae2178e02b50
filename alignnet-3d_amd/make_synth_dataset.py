#!/usr/bin/env python3
"""Make a SynthCars-style dataset on the GPU, in the reference's on-disk layout.

The reference's SynthCars / SynthCarsPersons / Synth20 datasets come from SyntheticScene.generate_pointcloud_embree
(tp_utils/pointcloud.py:1055-1186: trimesh + embree on ModelNet40Aligned meshes); here the scenes are drawn by alignnet3d/scenes.py in
the reference's np.random order (scene i is drawn from seed0 + i) and cast by the engine (csrc/alignnet_scene.hip).  The range noise is
the engine's counter stream, not np.random.randn's, so a dataset is distributed like the reference's, not equal to it.

    python make_synth_dataset.py --out data/SynthCars --kind cars --n-train 20000 --n-val 1000
    python make_synth_dataset.py --out data/Synth20 --kind cats --cats airplane,chair,sofa --meshes /data/ModelNet40Aligned

Written: meta/%08d.json (the keys of Scene.save_meta + SyntheticScene.save_meta), pointcloud{1,2}/%08d.npy (float64 [n, 3]),
transform/%08d.npy (rel_transform), split/train.txt, split/val.txt.  train.py, icp_global.py and icp_global_fast.py run on it as it is.
--meshes builtin (the default) uses the procedural car / person shapes of alignnet3d/scenes.py: no mesh files needed.
--cast scan|binned|auto (default scan) chooses how a cloud is cast (engine option "scene_cast"): `scan` runs every 8-column tile of a
cloud's azimuth window through the whole mesh, `binned` first bins the triangles to the tiles they can reach, and `auto` bins the meshes of more than 512 triangles.  All three write
the same files, bit for bit.  `binned` and `auto` are exact alternatives, not accelerations: measured on an MI355X the scan is the faster
one at every mesh size tried, 516 to 100,002 triangles (binned runs at 0.79 - 0.95 of its speed, profiles/scene_cast_rate.json), so keep
the default, also for --meshes DIR.
--rows runs the inner loop of the chosen cast by elevation band (engine option "scene_rows"): a triangle is intersected only with the
bands of 8 rows it can reach instead of all 64 rows of a tile.  The files are the same again.  Measured on an MI355X
(profiles/scene_rows_rate.json) it is ahead at every mesh size: 1.57 x for the built-in car with the default cast, and with --cast binned
-- which pays once the bands have cut the intersections -- 2.1 x at 5,001, 2.5 x at 20,001 and 2.7 x at 100,002 triangles: use --rows with
builtin meshes, --rows --cast binned with --meshes DIR.  Off by default.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHUNK = 256   # scenes per engine call


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True, help="dataset directory to write")
    ap.add_argument("--kind", choices=("cars", "carspersons", "cats"), default="cars")
    ap.add_argument("--meshes", default="builtin", help="'builtin' or the root of ModelNet40Aligned (<cat>/{train,test}/<cat>_%%04d.off)")
    ap.add_argument("--cats", default="car,person", help="comma-separated categories of --kind cats")
    ap.add_argument("--n-train", type=int, default=1000)
    ap.add_argument("--n-val", type=int, default=100)
    ap.add_argument("--seed0", type=int, default=0, help="scene i is drawn from seed0 + i")
    ap.add_argument("--second-object-set", action="store_true", help="the held-out mesh ids (pointcloud.py:1065-1075, 1181-1182)")
    ap.add_argument("--person-prob", type=float, default=0.2)
    ap.add_argument("--no-noise", action="store_true")
    ap.add_argument("--cast", choices=("scan", "binned", "auto"), default="scan",
                    help="scan: every tile goes through the whole mesh; binned: triangles binned to tiles first (same result, measured slower than scan); auto: binned above 512 triangles")
    ap.add_argument("--rows", action="store_true", help="run the chosen cast by elevation band inside a tile (engine option scene_rows; same result)")
    ap.add_argument("--device", type=int, default=0)
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.n_train < 0 or args.n_val < 0 or args.n_train + args.n_val < 1:
        ap.error("--n-train / --n-val: at least one scene")

    import alignnet3d
    from alignnet3d import scenes as S
    n = args.n_train + args.n_val
    scenes = [S.draw_scene(args.seed0 + i, args.kind, second_object_set=args.second_object_set, person_prob=args.person_prob,
                           cats=[c for c in args.cats.split(",") if c]) for i in range(n)]
    eng = alignnet3d.Engine(device=args.device)
    lib = S.MeshLibrary(args.meshes)
    t0 = time.perf_counter()
    hits = binned = 0
    for lo in range(0, n, CHUNK):
        part = scenes[lo:lo + CHUNK]
        off = S.generate(eng, part, seed=args.seed0, meshes=lib, noise=not args.no_noise, cast=args.cast, rows=args.rows)
        binned += eng.get_option("scene_binned_clouds")
        p1, p2 = eng.scene_read(off)
        hits += int(off[-1].sum())
        for i, s in enumerate(part):   # write_dataset numbers its examples from 0: hand it one scene at a time under its global index
            _write_one(S, args.out, lo + i, s, p1[off[i, 0]:off[i + 1, 0]], p2[off[i, 1]:off[i + 1, 1]])
    _write_split(args.out, args.n_train, n)
    eng.close()
    print("wrote %d scenes (%d train, %d val) to %s: %.1f points per cloud, %d distinct meshes, cast %s (%d of %d clouds binned)%s, %.2f s" %
          (n, args.n_train, args.n_val, args.out, hits / (2.0 * n), len(lib.meshes), args.cast, binned, 2 * n, " by elevation band" if args.rows else "",
           time.perf_counter() - t0))


def _write_one(S, root, index, scene, pc1, pc2):
    import json
    stem = str(index).zfill(8)
    for sub in ("meta", "pointcloud1", "pointcloud2", "transform", "split"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    with open(os.path.join(root, "meta", stem + ".json"), "w") as fh:
        json.dump(S.scene_meta(scene), fh)
    np.save(os.path.join(root, "pointcloud1", stem), np.asarray(pc1, np.float64))
    np.save(os.path.join(root, "pointcloud2", stem), np.asarray(pc2, np.float64))
    np.save(os.path.join(root, "transform", stem), scene.transform.rel_transform)


def _write_split(root, n_train, n):
    for name, ids in (("train", range(n_train)), ("val", range(n_train, n))):
        with open(os.path.join(root, "split", name + ".txt"), "w") as fh:
            fh.write("".join("%d\n" % i for i in ids))


if __name__ == "__main__":
    main()
