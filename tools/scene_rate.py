#!/usr/bin/env python3
"""GPU: throughput of the scene generator (csrc/alignnet_scene.hip) -- 256 scenes of the built-in car drawn at the reference's pose distribution
(alignnet3d/scenes.py draw_scene "cars": 4 - 20 m, scale 6), median of 5 calls, split into window / cast / compaction + noise by the engine's
kernel timers; the same with the noise off; the same against a 20000-triangle subdivision of the car, what a ModelNet-sized model costs; the
hits per cloud of the car at 4, 12 and 20 m; and the NumPy restatement's time per scene (tests/scene_ref.py) beside them.  Every configuration
runs in a child process of its own under a time limit.  Prints one JSON line.
Usage: python tools/scene_rate.py [scenes]"""
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
CONFIGS = ("car_noise", "car_clean", "car20k_noise")
LIMIT = 240   # seconds per child


def subdivide(v, f, target):
    """Midpoint subdivision (1 -> 4 triangles): whole passes while they stay under `target` faces, then the first faces one by one up to it."""
    v = list(map(tuple, np.asarray(v, np.float64))); f = [tuple(int(i) for i in t) for t in f]
    while len(f) < target:
        mid, nf = {}, []
        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                v.append(tuple((np.array(v[a]) + np.array(v[b])) / 2)); mid[k] = len(v) - 1
            return mid[k]
        split = len(f) if 4 * len(f) <= target else -(-(target - len(f)) // 3)
        for a, b, c in f[:split]:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf + f[split:]
    return np.array(v, np.float64), np.array(f, np.int32)


def child(config, B):
    import alignnet3d
    from alignnet3d import scenes as S
    scenes = [S.draw_scene(i, "cars") for i in range(B)]
    v, f, _ = S.load_mesh("builtin", "car", 1)
    if config.startswith("car20k"):
        v, f = subdivide(v, f, 20000)
    eng = alignnet3d.Engine()
    eng.scene_upload_meshes([(v, f, S.mesh_centroid(v, f))])
    poses = np.array([[list(s.transform.start_position) + [s.transform.start_angle], list(s.transform.end_position) + [s.transform.end_angle]] for s in scenes])
    args = dict(scene_ids=[s.seed for s in scenes], seed=0, sigma=0.05 if config.endswith("noise") else 0.0)
    run = lambda: eng.scene_generate([0] * B, [s.mesh_scale for s in scenes], poses, **args)
    off = run(); run()
    wall = []
    for _ in range(5):
        t = time.perf_counter(); run(); wall.append(time.perf_counter() - t)
    eng.profile_enable(True); eng.profile_read(reset=True)
    stages = {k: [] for k in ("scene_window", "scene_cast", "scene_compact")}
    for _ in range(5):
        run(); kern = eng.profile_kernels(); eng.profile_read(reset=True)
        for k in stages: stages[k].append(kern[k][0])
    eng.profile_enable(False)
    out = dict(config=config, scenes=B, triangles=int(len(f)), points_per_cloud=float(off[-1].sum()) / (2 * B), ms_per_call=float(np.median(wall)) * 1e3,
               scenes_per_s=B / float(np.median(wall)), **{k + "_ms": float(np.median(x)) for k, x in stages.items()})
    if config == "car_clean":   # hits per cloud by range, and the restatement's time per scene
        for dist in (4.0, 12.0, 20.0):
            p = [[(dist * np.sin(a), dist * np.cos(a), 0.0, yaw) for a, yaw in ((0.3, 0.0), (2.0, 1.0))] for _ in range(1)]
            o = eng.scene_generate([0], [6.0], p, sigma=0.0)
            out["hits_at_%dm" % dist] = [int(o[1, 0]), int(o[1, 1])]
        from tests import scene_ref as R
        t = time.perf_counter()
        for s in scenes[:4]:
            for q in poses[s.seed]:
                R.cloud(v, f, s.mesh_scale, q)
        out["restatement_s_per_scene"] = (time.perf_counter() - t) / 4
    eng.close()
    print("SCENE_RATE " + json.dumps(out), flush=True)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    res = {}
    for config in CONFIGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, str(B)], capture_output=True, text=True, timeout=LIMIT)
        line = [l for l in r.stdout.splitlines() if l.startswith("SCENE_RATE ")]
        if r.returncode != 0 or not line:
            sys.exit("scene_rate: %s failed (exit %d)\n%s" % (config, r.returncode, r.stderr[-3000:]))
        res[config] = json.loads(line[-1][len("SCENE_RATE "):])
    stamp = os.path.join(ROOT, ".build_commit")   # tools/gpu.sh writes it: the tree the numbers were taken at
    print(json.dumps(dict(tool="scene_rate", commit=open(stamp).read().strip() if os.path.exists(stamp) else None, **res)))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
