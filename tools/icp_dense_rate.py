# GPU: ICP on dense clouds -- the brute-force scan (icp_search 0) against the grid search (icp_search 1) on pairs from the scene generator at
# fixed sensor distances (about 4,266 / 6,000 / 13,700 / 58,600 target points; tools/icp_rate.py's own 1,500-point input beside them), radius 0.1,
# 30 iterations, both estimates.  Per size both options are warmed up, then timed alternately in this process: wall time of the whole call
# (upload of the inits, kernels, read-back, the stream synchronised inside it), median of 5.  Where the warm-up scan call took more than --slow
# seconds the timed calls are cut to ONE per option (printed and recorded); --pairs lowers the batch for the two largest sizes.
# The grid build's share and the candidates per query come from the library's own timers and read-back.  Writes profiles/icp_dense_rate.json.
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
import alignnet3d
from alignnet3d import scenes
from oracle import alignnet_ref as R
from oracle import icp_ref as I

LDS_BUDGET = 4266   # csrc/alignnet_icp.hip kIcpLdsBudget: where the scan leaves its LDS stage, and icp_search 2's threshold
p = argparse.ArgumentParser()
p.add_argument("--pairs", type=int, default=256)
p.add_argument("--pairs-large", type=int, default=256, help="pairs at the two largest sizes")
p.add_argument("--distances", default="14.5,11.8,8.0,4.0", help="sensor distances (m) of the generated scenes")
p.add_argument("--slow", type=float, default=6.0, help="a warm-up scan call longer than this (s) cuts the timed calls to one per option")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_dense_rate.json"))
a = p.parse_args()
eng = alignnet3d.Engine()
rng = np.random.default_rng(0)


def inits_of(trans, angle, centre):
    return [I.get_mat_angle(trans[i] + rng.normal(0, 0.05, 3), float(angle[i]) + rng.normal(0, 0.03), rotation_center=centre[i]) for i in range(len(trans))]


def measure(name, n, mean_n1, mean_n2, inits, first_pair):
    rows = np.arange(n)
    out = dict(input=name, pairs=n, mean_n1=mean_n1, mean_n2=mean_n2, estimates={})
    for constrained in (True, False):
        warm = {}
        for opt in (0, 1):
            eng.set_option("icp_search", opt)
            t = time.perf_counter(); eng.icp_refine_rows(rows, inits, 0.1, 30, constrained=constrained); warm[opt] = time.perf_counter() - t
        reps = 5 if warm[0] <= a.slow else 1
        ts, res = {0: [], 1: []}, {}
        for _ in range(reps):
            for opt in (0, 1):
                eng.set_option("icp_search", opt)
                t = time.perf_counter(); res[opt] = eng.icp_refine_rows(rows, inits, 0.1, 30, constrained=constrained); ts[opt].append(time.perf_counter() - t)
        eng.set_option("icp_search", 1)
        eng.profile_enable(True); eng.profile_read(reset=True)
        eng.icp_refine_rows(rows, inits, 0.1, 30, constrained=constrained)
        eng.synchronize()
        k = eng.profile_kernels(); eng.profile_read(reset=True); eng.profile_enable(False)
        build, loop = k.get("icp_grid_build", (0.0, 0))[0], k.get("icp_grid", (0.0, 0))[0]
        scan_ms, grid_ms = 1e3 * float(np.median(ts[0])), 1e3 * float(np.median(ts[1]))
        same = bool(np.array_equal(res[0]["fitness"], res[1]["fitness"]) and np.array_equal(res[0]["iterations"], res[1]["iterations"]))
        dT = float(np.abs(res[0]["transforms"] - res[1]["transforms"]).max())
        kind = "z-constrained" if constrained else "full rotation"
        print("%-22s %-13s %3d pairs, n2 %7.0f: scan %9.2f ms, grid %8.2f ms (%5.1fx; median of %d), grid build %.3f ms = %.1f %% of build + iterations (%.3f ms), "
              "mean iterations %.2f, fitness %.3f, same fitness / iterations %s, transforms differ by <= %.2g"
              % (name, kind, n, mean_n2, scan_ms, grid_ms, scan_ms / grid_ms, reps, build, 100 * build / max(build + loop, 1e-9), build + loop,
                 res[1]["iterations"].mean(), res[1]["fitness"].mean(), same, dT), flush=True)
        out["estimates"][kind] = dict(scan_ms=scan_ms, grid_ms=grid_ms, speedup=scan_ms / grid_ms, timed_calls_per_option=reps, warmup_scan_s=warm[0],
                                      grid_build_ms=build, grid_iterations_ms=loop, grid_build_share=build / max(build + loop, 1e-9),
                                      mean_iterations=float(res[1]["iterations"].mean()), mean_fitness=float(res[1]["fitness"].mean()),
                                      same_fitness_and_iterations=same, max_transform_difference=dT)
    d = eng.debug_icp_grid(first_pair[0], first_pair[1], inits[0], radius=0.1)
    out["candidates_per_query_pair0"] = float(d["candidates"].mean()); out["largest_bucket_pair0"] = d["largest_bucket"]; out["cell_edge"] = d["cell_edge"]
    print("%-22s pair 0: %.1f candidates per query (n2 %d), largest bucket %d, %d buckets occupied" % (name, d["candidates"].mean(), len(first_pair[1]), d["largest_bucket"], d["buckets_occupied"]), flush=True)
    return out


results = []
# tools/icp_rate.py's input: 1,500-point clouds
n, P = a.pairs, 1500
d = R.synth_pairs(n, P, dtype=np.float32)
off = np.zeros((n + 1, 2), np.int64); off[1:, 0] = off[1:, 1] = np.arange(1, n + 1) * P
eng.upload_dataset(d["pcs1"].reshape(-1, 3), d["pcs2"].reshape(-1, 3), off, np.zeros((n, 12), np.float32))
results.append(measure("synth_pairs 1500", n, P, P, inits_of(d["translations"], d["rel_angles"][:, 0], d["pc1_centers"]), (d["pcs1"][0], d["pcs2"][0])))
dists = [float(x) for x in a.distances.split(",")]
for di, dist in enumerate(dists):
    n = a.pairs_large if di >= len(dists) - 2 else a.pairs
    sc = [scenes.draw_scene(1000 + i, kind="cars", polar_dist_range=(dist, dist)) for i in range(n)]
    off = scenes.generate(eng, sc, seed=0, install=True)
    cnt = np.diff(off, axis=0)
    p1, p2 = eng.scene_read(off)
    lab = np.stack([scenes.scene_labels(s) for s in sc]).astype(np.float64)
    inits = inits_of(lab[:, 0:3], lab[:, 3], lab[:, 4:7])
    results.append(measure("scene at %.1f m" % dist, n, float(cnt[:, 0].mean()), float(cnt[:, 1].mean()), inits, (p1[: off[1, 0]], p2[: off[1, 1]])))
    results[-1]["distance_m"] = dist
faster = [r["mean_n2"] for r in results if all(e["speedup"] > 1.0 for e in r["estimates"].values())]
slower = [r["mean_n2"] for r in results if not all(e["speedup"] > 1.0 for e in r["estimates"].values())]
crossover = None if not faster else (min(faster) if not slower or max(slower) < min(faster) else None)
summary = dict(radius=0.1, iterations=30, lds_budget=LDS_BUDGET, auto_threshold=LDS_BUDGET, grid_faster_from_mean_n2=crossover,
               grid_faster_at_every_size_above_budget=all(all(e["speedup"] > 1.0 for e in r["estimates"].values()) for r in results if r["mean_n2"] > LDS_BUDGET),
               timing="wall time of one icp_refine_rows call (inits up, kernels, results down, stream synchronised), options timed alternately after a warm-up of each",
               results=results)
print("grid faster than the scan from a mean n2 of %s on (sizes measured: %s); automatic threshold %d" % (crossover, [round(r["mean_n2"]) for r in results], LDS_BUDGET))
os.makedirs(os.path.dirname(a.out), exist_ok=True)
json.dump(summary, open(a.out, "w"), indent=1)
eng.close()
