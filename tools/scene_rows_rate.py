#!/usr/bin/env python3
"""GPU: the scene generator's cast by elevation band (engine option scene_rows) against the whole-tile inner loop, under both stagings -- four
settings: scan and binned (scene_cast 0 / 1), each with scene_rows 0 and 1 -- on the built-in car (516 triangles) and its midpoint subdivisions to
5,001, 20,001 and 100,002 triangles, 256 scenes (512 clouds) at the reference's pose distribution (alignnet3d/scenes.py draw_scene "cars": 4 - 20 m,
scale 6), noise on: tools/scene_cast_rate.py's workload.  Per mesh every setting is warmed up (and its offsets and clouds compared with the
baseline's: they must be equal bit for bit), then the four are timed alternately in one process: wall time of the whole alignnet_scene_generate call
(uploads, kernels, the window / list-size copies, the stream synchronised inside it), median of 5 with min .. max.  The BASELINE is scene_cast 0 with
scene_rows 0 in the same run: the kernels as they were before the option existed.  Per setting also: the kernel-timer split (cast = "scene_cast" or
"scene_band", binning = "scene_bin"), and cells per entry -- over the first 64 clouds, the set band bits of the staged triangles (the band read-back's
total) over the entries of the tile lists (the binned read-back's; the scan's side tests leave it about the same entries): 8 would be
every band of every entry, i.e. the whole-tile loop's work.  Every mesh size runs in a child process under a time limit; the parent stops at the
first child that fails.  Writes profiles/scene_rows_rate.json; --markdown FILE prints the DESIGN.md table and the README row from such a file.
Usage: python tools/scene_rows_rate.py [--scenes 256] [--sizes 516,5000,20000,100000] [--out FILE] | --markdown FILE"""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300          # seconds per child
SETTINGS = ((0, 0), (1, 0), (0, 1), (1, 1))      # (scene_cast, scene_rows); the first is the baseline
NAMES = {(0, 0): "scan", (1, 0): "binned", (0, 1): "scan+rows", (1, 1): "binned+rows"}
STAGES = ("scene_window", "scene_bin", "scene_cast", "scene_band", "scene_compact")


def child(target, B):
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

    def run(setting):
        eng.set_option("scene_cast", setting[0]); eng.set_option("scene_rows", setting[1])
        t = time.perf_counter()
        off = eng.scene_generate([0] * B, scale, poses, scene_ids=[s.seed for s in scenes], seed=0, sigma=0.05)
        return time.perf_counter() - t, off

    base = None
    for s in SETTINGS:
        off = run(s)[1]
        got = (off, *eng.scene_read(off))
        if base is None:
            base = got
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), "%s returned other offsets or clouds than the baseline at %d triangles" % (NAMES[s], len(f))
    points = float(base[0][-1].sum()) / (2 * B)
    del base, got
    ts = {s: [] for s in SETTINGS}
    for _ in range(5):
        for s in SETTINGS:
            ts[s].append(run(s)[0])
    kernels = {}
    eng.profile_enable(True); eng.profile_read(reset=True)
    for s in SETTINGS:
        acc = {k: [] for k in STAGES}
        for _ in range(3):
            run(s); kern = eng.profile_kernels(); eng.profile_read(reset=True)
            for k in STAGES: acc[k].append(kern.get(k, (0.0, 0))[0])
        med = {k: float(np.median(x)) for k, x in acc.items()}
        kernels[s] = dict(cast_ms=med["scene_cast"] + med["scene_band"], binning_ms=med["scene_bin"], window_ms=med["scene_window"], compact_ms=med["scene_compact"])
    eng.profile_enable(False)
    eng.set_option("scene_cast", 0); eng.set_option("scene_rows", 0)
    # cells per entry over the first 64 clouds (the read-backs cast one cloud per call)
    entries = cells_scan = cells_list = 0
    for s, p in zip(scenes[:32], poses[:32]):
        for q in p:
            entries += eng.debug_scene_cast(0, s.mesh_scale, q, binned=True)["entries"]
            cells_scan += eng.debug_scene_cast(0, s.mesh_scale, q, rows=True)["cells"]
            cells_list += eng.debug_scene_cast(0, s.mesh_scale, q, binned=True, rows=True)["cells"]
    eng.close()
    res = dict(triangles=int(len(f)), scenes=B, clouds=2 * B, points_per_cloud=points, timed_calls_per_setting=5, entries_first_64_clouds=int(entries), settings={})
    b_ms, b_min, b_max = 1e3 * float(np.median(ts[0, 0])), 1e3 * min(ts[0, 0]), 1e3 * max(ts[0, 0])
    for s in SETTINGS:
        ms = 1e3 * float(np.median(ts[s]))
        cells = None if not s[1] else (cells_list if s[0] else cells_scan)
        res["settings"][NAMES[s]] = dict(scene_cast=s[0], scene_rows=s[1], ms=ms, ms_min=1e3 * min(ts[s]), ms_max=1e3 * max(ts[s]), speedup=b_ms / ms,
                                         ahead_beyond_spread=bool(1e3 * max(ts[s]) < b_min), behind_beyond_spread=bool(1e3 * min(ts[s]) > b_max),
                                         cells_first_64_clouds=cells, cells_per_entry=8.0 if cells is None else (cells / entries if entries else 0.0), **kernels[s])
    print("SCENE_ROWS_RATE " + json.dumps(res), flush=True)


def markdown(path):
    d = json.load(open(path))
    fmt = lambda s: "%.2f (%.2f .. %.2f)" % (s["ms"], s["ms_min"], s["ms_max"])
    print("| triangles | scan, ms | binned, ms | scan + rows, ms | x | binned + rows, ms | x | cast kernels, ms (same order) | binning, ms | cells per entry (scan / list staging) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in d["results"]:
        s = r["settings"]
        print("| %s | %s | %s | %s | %.2f | %s | %.2f | %s | %.2f | %.2f / %.2f |" %
              (format(r["triangles"], ","), fmt(s["scan"]), fmt(s["binned"]), fmt(s["scan+rows"]), s["scan+rows"]["speedup"], fmt(s["binned+rows"]),
               s["binned+rows"]["speedup"], " / ".join("%.2f" % s[k]["cast_ms"] for k in ("scan", "binned", "scan+rows", "binned+rows")),
               s["binned+rows"]["binning_ms"], s["scan+rows"]["cells_per_entry"], s["binned+rows"]["cells_per_entry"]))
    print()
    best = []
    for r in d["results"]:
        ahead = {k: v for k, v in r["settings"].items() if v["ahead_beyond_spread"]}
        k = max(ahead, key=lambda k: ahead[k]["speedup"]) if ahead else None
        best.append("%s: %s" % (format(r["triangles"], ","), "none ahead" if k is None else "%s %.2f x (%.2f -> %.2f ms)" % (k, ahead[k]["speedup"], r["settings"]["scan"]["ms"], ahead[k]["ms"])))
    print("README row: " + "; ".join(best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--sizes", default="516,5000,20000,100000", help="triangles: the built-in car (516) and subdivisions of it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_rows_rate.json"))
    ap.add_argument("--markdown", metavar="FILE", help="print the DESIGN.md table and the README row from a result file; nothing is run")
    a = ap.parse_args()
    if a.markdown:
        return markdown(a.markdown)
    commit = None
    if os.path.exists(os.path.join(ROOT, ".build_commit")):
        commit = open(os.path.join(ROOT, ".build_commit")).read().strip()
    results, stopped = [], None
    for size in [int(x) for x in a.sizes.split(",")]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(size), str(a.scenes)], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            stopped = "%d triangles ran into the time limit of %d s" % (size, LIMIT)
            break
        line = [l for l in r.stdout.splitlines() if l.startswith("SCENE_ROWS_RATE ")]
        if r.returncode != 0 or not line:
            stopped = "%d triangles failed (exit %d)" % (size, r.returncode)
            print(r.stderr[-3000:], file=sys.stderr)
            break
        res = json.loads(line[-1][len("SCENE_ROWS_RATE "):])
        results.append(res)
        print("%7d triangles: " % res["triangles"] + "; ".join("%s %.2f ms (%.2f .. %.2f) %.2fx, cast %.2f + binning %.2f ms, %.2f cells/entry" %
              (k, s["ms"], s["ms_min"], s["ms_max"], s["speedup"], s["cast_ms"], s["binning_ms"], s["cells_per_entry"]) for k, s in res["settings"].items()), flush=True)
    summary = dict(tool="scene_rows_rate", commit=commit, stopped=stopped,
                   timing="wall time of one alignnet_scene_generate call (uploads, kernels, window and list-size copies, stream synchronised), the four settings "
                          "timed alternately after a warm-up of each, median of 5; baseline = scene_cast 0, scene_rows 0 of the same run; ahead = the setting's "
                          "slowest timed call is faster than the baseline's fastest; cells per entry = set band bits of staged triangles / tile-list entries, first "
                          "64 clouds (8 = the whole-tile loop)",
                   results=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(summary, open(a.out, "w"), indent=1)
    if stopped:   # what was measured before is written; nothing further was started
        sys.exit("scene_rows_rate: " + stopped + "; stopped")


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
