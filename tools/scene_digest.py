#!/usr/bin/env python3
"""GPU: SHA-256 digests of everything the scene generator's cast returns, one line each, for comparing two builds of the library bit for bit
(ALIGNNET_HIP_LIB selects the library; run once per build, each run a process of its own, and diff the listings).
Records: every case of tests/scene_rows_cases.py (OLD_NAMES + NAMES, each with its own sensor tables) through debug_scene_cast under plain, binned,
rows and binned + rows, at lds_triangles 0 and 17: the window, t, triangle, and tile_counts / cell_counts where the read-back returns them.
Batch: tests/scene_cases.BATCH through scene_generate (seed 7, sigma 0.05, clip 0.05) under all six (scene_cast, scene_rows) settings: the offsets
and both point blobs.  fp64 in a fixed order: tolerance plays no part, every line of two builds that compute the same must be equal.
Usage: python tools/scene_digest.py [--out FILE]"""
import argparse, hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)


def sha(x, dtype):
    return hashlib.sha256(np.ascontiguousarray(x, dtype).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the listing to this file")
    a = ap.parse_args()
    import alignnet3d
    from alignnet3d import scenes as S
    from tests import scene_cases as C
    from tests import scene_rows_cases as RC
    from tests.helpers import small_cfg
    lines = []

    def emit(key, digest):
        lines.append("%s %s" % (digest, key)); print(lines[-1], flush=True)

    eng = alignnet3d.Engine(small_cfg(N=64, nb=12))
    for name in RC.OLD_NAMES + RC.NAMES:
        v, f, scale, pose = RC.case(name)
        eng.scene_upload_meshes([(v, f, S.mesh_centroid(v, f))], sensor=RC.tables(name))
        for binned in (False, True):
            for rows in (False, True):
                for lds in (0, 17):
                    rec = eng.debug_scene_cast(0, scale, pose, lds_triangles=lds, binned=binned, rows=rows)
                    key = "record %s %s lds=%d" % (name, {(False, False): "plain", (True, False): "binned", (False, True): "rows", (True, True): "binned+rows"}[binned, rows], lds)
                    emit(key + " window", sha(rec["window"], np.int64))
                    emit(key + " t", sha(rec["t"], np.float64))
                    emit(key + " triangle", sha(rec["triangle"], np.int32))
                    for extra in ("tile_counts", "cell_counts"):
                        if extra in rec:
                            emit(key + " " + extra, sha(rec[extra], np.int64))
    names = sorted(C.BATCH_MESHES)
    meshes = [C.BATCH_MESHES[n]() for n in names]
    eng.scene_upload_meshes([(v, f, S.mesh_centroid(v, f)) for v, f in meshes])
    for cast in (0, 1, 2):
        for rows in (0, 1):
            eng.set_option("scene_cast", cast); eng.set_option("scene_rows", rows)
            off = eng.scene_generate([names.index(b[0]) for b in C.BATCH], [b[1] for b in C.BATCH], [[b[2], b[3]] for b in C.BATCH],
                                     scene_ids=[b[4] for b in C.BATCH], seed=7, sigma=0.05, clip=0.05)
            p1, p2 = eng.scene_read(off)
            key = "batch scene_cast=%d scene_rows=%d" % (cast, rows)
            emit(key + " offsets", sha(off, np.int64))
            emit(key + " points1", sha(p1, np.float32))
            emit(key + " points2", sha(p2, np.float32))
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
