# GPU: multi-scale ICP (Engine.icp_multiscale_refine_rows) beside the single-scale call with the grid search (icp_search 1: what there was for this work
# before) -- tools/icp_plane_rate.py's 256 pairs of 1,500 points and scenes from the generator at fixed sensor distances, from three starts: the truth
# disturbed by N(0, 0.05 m) per axis / N(0, 0.03 rad) (that tool's), the truth turned by 15 degrees and shifted 0.4 m (wide), and the centroid start.
# The schedule is an EXAMPLE, not a recommendation: voxels (0.2, 0.1, 0), radii (0.4, 0.2, 0.1), 30 iterations per level; single scale: radius 0.1, 30.
# Both calls are warmed up, then timed alternately in this process: wall time of the whole call, median of 5 with min .. max.  Beside the times: the
# pyramid's share (the library's device timers, "icp_pyramid"), level sizes, iterations per level, the share of pairs at a level's iteration limit,
# median and 90th-percentile translation and yaw error against the truth for both, and the pairs that end farther from the truth than single scale.
# All three starts for the point estimate; plane and generalized once, from the disturbed start.  Writes profiles/icp_multiscale_rate.json.
# --sync-probe: a warm-up call and --probe-calls steady-state multi-scale calls on the first input and nothing else, for rocprofv3 --hip-trace
# --kernel-trace --stats runs of their own: the hipStreamSynchronize calls of one steady-state call are the difference of the counts of two such runs
# divided by the difference of their --probe-calls; --sync-count N records the number read there in the profile.
import argparse, json, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
import alignnet3d
from alignnet3d import scenes
from oracle import alignnet_ref as R
from oracle import icp_ref as I

p = argparse.ArgumentParser()
p.add_argument("--pairs", type=int, default=256)
p.add_argument("--distances", default="14.5,8.0", help="sensor distances (m) of the generated scenes")
p.add_argument("--voxels", default="0.2,0.1,0")
p.add_argument("--radii", default="0.4,0.2,0.1")
p.add_argument("--its", default="30,30,30")
p.add_argument("--normal-radius", type=float, default=0.3)
p.add_argument("--sync-probe", action="store_true")
p.add_argument("--probe-calls", type=int, default=1)
p.add_argument("--sync-count", type=int, default=-1, help="hipStreamSynchronize calls of one steady-state call, as read from a trace of --sync-probe")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_multiscale_rate.json"))
a = p.parse_args()
VOX, RAD, ITS = [float(x) for x in a.voxels.split(",")], [float(x) for x in a.radii.split(",")], [int(x) for x in a.its.split(",")]
eng = alignnet3d.Engine()
eng.set_option("icp_search", 1)
rng = np.random.default_rng(0)
SINGLE = {"point": eng.icp_refine_rows, "plane": eng.icp_plane_refine_rows, "generalized": eng.icp_generalized_refine_rows}


def errors(T, truth, centre):
    """yaw error (degrees) and translation error at the cloud centre (m), per pair."""
    D = T @ np.linalg.inv(truth)
    c = np.concatenate([centre, np.ones((len(centre), 1))], 1)[:, :, None]
    return np.abs(np.degrees(np.arctan2(D[:, 1, 0], D[:, 0, 0]))), np.linalg.norm(((T - truth) @ c)[:, :3, 0], axis=1)


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * float(np.min(ts)), max_ms=1e3 * float(np.max(ts)))


def quality(T, truth, centre):
    yaw, tr = errors(T, truth, centre)
    return dict(yaw_deg_median=float(np.median(yaw)), yaw_deg_p90=float(np.percentile(yaw, 90)), translation_m_median=float(np.median(tr)),
                translation_m_p90=float(np.percentile(tr, 90))), tr


def compare(name, start, estimate, rows, inits, truth, centre):
    kw = {} if estimate == "point" else dict(normal_radius=a.normal_radius)
    single = lambda: SINGLE[estimate](rows, inits, radius=0.1, its=30, **kw)
    multi = lambda: eng.icp_multiscale_refine_rows(rows, inits, VOX, RAD, ITS, estimate=estimate, normal_radius=a.normal_radius)
    single(); multi()
    ts, res = {"single": [], "multi": []}, {}
    for _ in range(5):
        for key, fn in (("single", single), ("multi", multi)):
            t = time.perf_counter(); res[key] = fn(); ts[key].append(time.perf_counter() - t)
    eng.profile_enable(True); eng.profile_read(reset=True)
    multi(); eng.synchronize()
    kern = eng.profile_kernels(); eng.profile_read(reset=True); eng.profile_enable(False)
    pyramid_ms = kern.get("icp_pyramid", (0.0, 0))[0]
    qs, trs = quality(res["single"]["transforms"], truth, centre)
    qm, trm = quality(res["multi"]["transforms"], truth, centre)
    it, sz = res["multi"]["iterations"], res["multi"]["level_sizes"]
    worse = np.flatnonzero(trm > trs)
    y0, t0 = errors(np.stack(inits), truth, centre)
    rec = dict(input=name, start=start, estimate=estimate, pairs=len(rows), init_yaw_deg_median=float(np.median(y0)), init_translation_m_median=float(np.median(t0)),
               single=dict(stats(ts["single"]), mean_iterations=float(res["single"]["iterations"].mean()), share_at_limit=float((res["single"]["iterations"] >= 30).mean()),
                           mean_fitness=float(res["single"]["fitness"].mean()), **qs),
               multi=dict(stats(ts["multi"]), pyramid_device_ms=pyramid_ms, pyramid_share_of_call=pyramid_ms / (1e3 * float(np.median(ts["multi"]))),
                          workspace_bytes=eng.get_option("icp_multiscale_ws_bytes"), mean_level_sizes=sz.mean(0).tolist(), mean_iterations_per_level=it.mean(0).tolist(),
                          share_at_limit_per_level=[float((it[:, l] >= ITS[l]).mean()) for l in range(len(ITS))], mean_fitness_last_level=float(res["multi"]["fitness"].mean()), **qm),
               multi_over_single_time=float(np.median(ts["multi"]) / np.median(ts["single"])), multi_worse_than_single_pairs=int(worse.size),
               multi_worse_by_m_max=float((trm - trs)[worse].max()) if worse.size else 0.0)
    print("%-18s %-9s %-11s single %9.2f ms (%.2f .. %.2f) its %5.2f at limit %5.1f %% | multi %9.2f ms (%.2f .. %.2f) pyramid %.3f ms, its/level %s at limit %s, sizes %s"
          % (name, start, estimate, rec["single"]["median_ms"], rec["single"]["min_ms"], rec["single"]["max_ms"], rec["single"]["mean_iterations"], 100 * rec["single"]["share_at_limit"],
             rec["multi"]["median_ms"], rec["multi"]["min_ms"], rec["multi"]["max_ms"], pyramid_ms, ["%.1f" % x for x in it.mean(0)],
             ["%.0f %%" % (100 * x) for x in rec["multi"]["share_at_limit_per_level"]], [[round(x) for x in r] for r in sz.mean(0)]), flush=True)
    print("%-18s %-9s %-11s translation error m: single median %.4f p90 %.4f | multi median %.4f p90 %.4f; yaw deg: single %.3f p90 %.3f | multi %.3f p90 %.3f; "
          "multi ends farther from the truth on %d of %d pairs" % (name, start, estimate, qs["translation_m_median"], qs["translation_m_p90"], qm["translation_m_median"],
                                                                   qm["translation_m_p90"], qs["yaw_deg_median"], qs["yaw_deg_p90"], qm["yaw_deg_median"], qm["yaw_deg_p90"], worse.size, len(rows)), flush=True)
    return rec


def measure(name, n, trans, angle, centre, p1, p2, off):
    rows = np.arange(n)
    truth = np.stack([I.get_mat_angle(trans[i], float(angle[i]), rotation_center=centre[i]) for i in range(n)])
    starts = {"disturbed": [I.get_mat_angle(trans[i] + rng.normal(0, 0.05, 3), float(angle[i]) + rng.normal(0, 0.03), rotation_center=centre[i]) for i in range(n)]}
    if a.sync_probe:
        multi = lambda: eng.icp_multiscale_refine_rows(rows, starts["disturbed"], VOX, RAD, ITS)
        multi()               # the first call grows the workspaces
        for _ in range(a.probe_calls):
            multi()
        return []
    wide = []
    for i in range(n):
        d = rng.uniform(0, 2 * np.pi)
        wide.append(I.get_mat_angle(trans[i] + 0.4 * np.array([np.cos(d), np.sin(d), 0.0]), float(angle[i]) + np.deg2rad(15.0) * rng.choice([-1.0, 1.0]), rotation_center=centre[i]))
    starts["wide"] = wide
    starts["centroid"] = list(eng.centroid_inits(p1, p2, off, rows))
    out = [compare(name, s, "point", rows, starts[s], truth, centre) for s in ("disturbed", "wide", "centroid")]
    out += [compare(name, "disturbed", e, rows, starts["disturbed"], truth, centre) for e in ("plane", "generalized")]
    return out


results = []
n, P = a.pairs, 1500
d = R.synth_pairs(n, P, dtype=np.float32)
off = np.zeros((n + 1, 2), np.int64); off[1:, 0] = off[1:, 1] = np.arange(1, n + 1) * P
eng.upload_dataset(d["pcs1"].reshape(-1, 3), d["pcs2"].reshape(-1, 3), off, np.zeros((n, 12), np.float32))
results += measure("synth_pairs 1500", n, d["translations"].astype(np.float64), d["rel_angles"][:, 0].astype(np.float64), d["pc1_centers"].astype(np.float64),
                   d["pcs1"].reshape(-1, 3), d["pcs2"].reshape(-1, 3), off)
if a.sync_probe:
    eng.close()
    sys.exit(0)
for dist in [float(x) for x in a.distances.split(",")]:
    sc = [scenes.draw_scene(1000 + i, kind="cars", polar_dist_range=(dist, dist)) for i in range(n)]
    off = scenes.generate(eng, sc, seed=0, install=True)
    p1, p2 = eng.scene_read(off)
    lab = np.stack([scenes.scene_labels(s) for s in sc]).astype(np.float64)
    results += measure("scene at %.1f m" % dist, n, lab[:, 0:3], lab[:, 3], lab[:, 4:7], p1, p2, off)
remarks = os.path.join(ROOT, "alignnet-3d_amd", "csrc", "alignnet_multiscale.remarks")
kernels = {}
if os.path.exists(remarks):
    for m in re.finditer(r"Function Name: \S*?(ms_\w+_kernel)\S*.*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)",
                         open(remarks).read(), re.S):
        kernels[m.group(1)] = dict(vgprs=int(m.group(2)), scratch_bytes=int(m.group(3)), occupancy_waves_per_simd=int(m.group(4)), static_lds_bytes=int(m.group(5)))
summary = dict(schedule=dict(voxel_sizes=VOX, radii=RAD, its=ITS, note="an example, not a recommendation"), single="radius 0.1, 30 iterations, icp_search 1 (grid)",
               normal_radius=a.normal_radius, stream_synchronisations_per_call=a.sync_count if a.sync_count >= 0 else None,
               timing="wall time of one call (inits up, kernels, results down), the two calls timed alternately after a warm-up of each; median of 5",
               pyramid="device time of the three pyramid kernels of one call (the library's event timers)", kernels=kernels, results=results)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
json.dump(summary, open(a.out, "w"), indent=1)
eng.close()
