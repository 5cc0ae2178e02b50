#!/usr/bin/env python3
"""GPU: the scene generator's two casts side by side -- the scan (scene_cast 0: every tile of a cloud's window goes through the whole mesh) against
the binned cast (scene_cast 1: triangles binned to the tiles first) -- on the built-in car (516 triangles) and its midpoint subdivisions to 5,000,
20,000 and 100,000 triangles, 256 scenes (512 clouds) at the reference's pose distribution (alignnet3d/scenes.py draw_scene "cars": 4 - 20 m, scale 6),
noise on.  Per mesh both options are warmed up (and their offsets and clouds compared: they must be equal bit for bit), then timed alternately in one
process: wall time of the whole alignnet_scene_generate call (uploads, kernels, the window / list-size copies, the stream synchronised inside it),
median of 5 with the min / max spread.  Where the scan's warm-up call took more than --slow seconds the timed calls are cut to ONE per option
(recorded).  Kernel times per stage come from the engine's timers, the list sizes from its counters and the binned read-back.  Every mesh size runs
in a child process of its own under a time limit; the parent stops at the first child that fails.  Writes profiles/scene_cast_rate.json.
Usage: python tools/scene_cast_rate.py [--scenes 256] [--sizes 516,5000,20000,100000] [--out FILE]"""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIMIT = 420          # seconds per child


def auto_threshold():
    """kSceneBinAuto as csrc/alignnet_scene.hip defines it (directly, or as kLdsTriangles)."""
    import re
    src = open(os.path.join(ROOT, "alignnet-3d_amd", "csrc", "alignnet_scene.hip")).read()
    v = re.search(r"constexpr int kSceneBinAuto = (\w+);", src).group(1)
    return int(v) if v.isdigit() else int(re.search(r"constexpr int %s = (\d+);" % v, src).group(1))


STAGES = ("scene_window", "scene_bin", "scene_cast", "scene_compact")


def child(target, B, slow):
    import alignnet3d
    from alignnet3d import scenes as S
    from scene_rate import subdivide
    scenes = [S.draw_scene(i, "cars") for i in range(B)]
    v, f, _ = S.load_mesh("builtin", "car", 1)
    if target > len(f):
        v, f = subdivide(v, f, target)
    eng = alignnet3d.Engine()
    eng.scene_upload_meshes([(v, f, S.mesh_centroid(v, f))])
    poses = np.array([[list(s.transform.start_position) + [s.transform.start_angle], list(s.transform.end_position) + [s.transform.end_angle]] for s in scenes])
    scale = [s.mesh_scale for s in scenes]

    def run(opt):
        eng.set_option("scene_cast", opt)
        t = time.perf_counter()
        off = eng.scene_generate([0] * B, scale, poses, scene_ids=[s.seed for s in scenes], seed=0, sigma=0.05)
        return time.perf_counter() - t, off

    warm, first = {}, {}
    for opt in (0, 1):
        warm[opt], off = run(opt)
        first[opt] = (off, *eng.scene_read(off))
    same = bool(np.array_equal(first[0][0], first[1][0]) and np.array_equal(first[0][1], first[1][1]) and np.array_equal(first[0][2], first[1][2]))
    assert same, "scene_cast 0 and 1 returned different offsets or clouds at %d triangles" % len(f)
    assert eng.get_option("scene_binned_clouds") == 2 * B
    entries = eng.get_option("scene_bin_entries")
    points = float(first[0][0][-1].sum()) / (2 * B)
    del first
    reps = 5 if warm[0] <= slow else 1
    ts = {0: [], 1: []}
    for _ in range(reps):
        for opt in (0, 1):
            ts[opt].append(run(opt)[0])
    stages = {}
    eng.profile_enable(True); eng.profile_read(reset=True)
    for opt in (0, 1):
        acc = {k: [] for k in STAGES}
        for _ in range(min(reps, 3)):
            run(opt); kern = eng.profile_kernels(); eng.profile_read(reset=True)
            for k in STAGES: acc[k].append(kern.get(k, (0.0, 0))[0])
        stages[opt] = {k + "_ms": float(np.median(x)) for k, x in acc.items()}
    eng.profile_enable(False)
    # the longest tile list among the first 32 scenes' clouds (the binned read-back, one cloud per call)
    longest, tiles = 0, 0
    for s, p in zip(scenes[:32], poses[:32]):
        for q in p:
            d = eng.debug_scene_cast(0, s.mesh_scale, q, binned=True)
            longest = max(longest, int(d["tile_counts"].max()) if len(d["tile_counts"]) else 0); tiles += len(d["tile_counts"])
    eng.close()
    ms = {o: 1e3 * float(np.median(ts[o])) for o in ts}
    out = dict(triangles=int(len(f)), scenes=B, clouds=2 * B, points_per_cloud=points, timed_calls_per_option=reps, warmup_scan_s=warm[0], warmup_binned_s=warm[1],
               scan_ms=ms[0], scan_ms_min=1e3 * min(ts[0]), scan_ms_max=1e3 * max(ts[0]), binned_ms=ms[1], binned_ms_min=1e3 * min(ts[1]), binned_ms_max=1e3 * max(ts[1]),
               speedup=ms[0] / ms[1], binned_ahead_beyond_spread=bool(max(ts[1]) < min(ts[0])), scan_kernels=stages[0], binned_kernels=stages[1],
               entries_per_cloud=entries / (2.0 * B), entries_per_triangle=entries / (2.0 * B * len(f)), longest_tile_list_first_64_clouds=longest,
               tiles_per_cloud_first_64_clouds=tiles / 64.0, equal_offsets_and_clouds=same)
    print("SCENE_CAST_RATE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--sizes", default="516,5000,20000,100000", help="triangles: the built-in car (516) and subdivisions of it")
    ap.add_argument("--slow", type=float, default=8.0, help="a warm-up scan call longer than this (s) cuts the timed calls to one per option")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_cast_rate.json"))
    a = ap.parse_args()
    AUTO_THRESHOLD = auto_threshold()
    commit = None
    if os.path.exists(os.path.join(ROOT, ".build_commit")):
        commit = open(os.path.join(ROOT, ".build_commit")).read().strip()
    results, stopped = [], None
    for size in [int(x) for x in a.sizes.split(",")]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(size), str(a.scenes), str(a.slow)], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            stopped = "%d triangles ran into the time limit of %d s" % (size, LIMIT)
            break
        line = [l for l in r.stdout.splitlines() if l.startswith("SCENE_CAST_RATE ")]
        if r.returncode != 0 or not line:
            stopped = "%d triangles failed (exit %d)" % (size, r.returncode)
            print(r.stderr[-3000:], file=sys.stderr)
            break
        res = json.loads(line[-1][len("SCENE_CAST_RATE "):])
        results.append(res)
        print("%7d triangles: scan %9.2f ms (%.2f .. %.2f), binned %8.2f ms (%.2f .. %.2f), %5.2fx, median of %d; cast kernel %.2f -> %.2f ms, binning %.2f ms; "
              "%.0f entries per cloud (%.2f per triangle), longest list %d" %
              (res["triangles"], res["scan_ms"], res["scan_ms_min"], res["scan_ms_max"], res["binned_ms"], res["binned_ms_min"], res["binned_ms_max"], res["speedup"],
               res["timed_calls_per_option"], res["scan_kernels"]["scene_cast_ms"], res["binned_kernels"]["scene_cast_ms"], res["binned_kernels"]["scene_bin_ms"],
               res["entries_per_cloud"], res["entries_per_triangle"], res["longest_tile_list_first_64_clouds"]), flush=True)
    ahead = [r["triangles"] for r in results if r["binned_ahead_beyond_spread"]]
    behind = [r["triangles"] for r in results if not r["binned_ahead_beyond_spread"]]
    crossover = None if not ahead else (min(ahead) if not behind or max(behind) < min(ahead) else None)
    summary = dict(tool="scene_cast_rate", commit=commit, auto_threshold=AUTO_THRESHOLD, binned_ahead_from_triangles=crossover, stopped=stopped,
                   timing="wall time of one alignnet_scene_generate call (uploads, kernels, window and list-size copies, stream synchronised), options timed "
                          "alternately after a warm-up of each; ahead = the binned call's slowest timed call is faster than the scan's fastest",
                   results=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(summary, open(a.out, "w"), indent=1)
    print("binned ahead of the scan beyond the spread from %s triangles on (sizes measured: %s); automatic threshold %d" % (crossover, [r["triangles"] for r in results], AUTO_THRESHOLD))
    if stopped:   # what was measured before is written; nothing further was started
        sys.exit("scene_cast_rate: " + stopped + "; stopped")


if __name__ == "__main__":
    if len(sys.argv) > 4 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]))
    else:
        main()
