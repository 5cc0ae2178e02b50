# GPU: generalized ICP (Engine.icp_generalized_refine_rows) beside point-to-point ICP with the grid search (icp_search 1) and point-to-plane ICP --
# the inputs, pairs and disturbed starts of tools/icp_plane_rate.py: 256 pairs of 1,500 points and scenes from the generator at fixed sensor distances,
# radius 0.1, normal radius 0.3, 30 iterations at most, both estimates, from the truth disturbed by N(0, 0.05 m) per axis and N(0, 0.03 rad) (the same
# generator and seed, drawn in the same order, so the starts are that tool's).  All three are warmed up, then timed alternately in this process: wall
# time of the whole call (inits up, kernels, results down, the stream synchronised inside it), median of 5 with min .. max.
# Beside the times, for point-to-plane and generalized: iterations used, the share of pairs at the iteration limit, the final yaw and translation error
# against the truth (the translation error is taken at the source cloud's centre; median and 90th percentile), the pairs where the estimate ends farther
# from the truth than point-to-point (and, for generalized, than point-to-plane), and the normals stage alone from the library's own timers
# ("icp_plane_normals": the target's bucket ordering + normals; "icp_generalized_normals": both clouds') beside the grid builds and the iterations.
# Writes profiles/icp_generalized_rate.json.
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
import alignnet3d
from alignnet3d import scenes
from oracle import alignnet_ref as R
from oracle import icp_ref as I

p = argparse.ArgumentParser()
p.add_argument("--pairs", type=int, default=256)
p.add_argument("--distances", default="14.5,8.0", help="sensor distances (m) of the generated scenes")
p.add_argument("--normal-radius", type=float, default=0.3)
p.add_argument("--its", type=int, default=30)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_generalized_rate.json"))
a = p.parse_args()
eng = alignnet3d.Engine()
eng.set_option("icp_search", 1)
rng = np.random.default_rng(0)
KEYS = ("point", "plane", "generalized")
TIMERS = {"plane": ("icp_grid_build", "icp_plane_normals", "icp_plane"), "generalized": ("icp_grid_build", "icp_generalized_normals", "icp_generalized")}


def errors(T, truth, centre):
    """yaw error (degrees) and translation error at the cloud centre (m), per pair."""
    D = T @ np.linalg.inv(truth)
    c = np.concatenate([centre, np.ones((len(centre), 1))], 1)[:, :, None]
    return np.abs(np.degrees(np.arctan2(D[:, 1, 0], D[:, 0, 0]))), np.linalg.norm(((T - truth) @ c)[:, :3, 0], axis=1)


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * float(np.min(ts)), max_ms=1e3 * float(np.max(ts)))


def measure(name, n, mean_n1, mean_n2, trans, angle, centre):
    rows = np.arange(n)
    truth = np.stack([I.get_mat_angle(trans[i], float(angle[i]), rotation_center=centre[i]) for i in range(n)])
    inits = [I.get_mat_angle(trans[i] + rng.normal(0, 0.05, 3), float(angle[i]) + rng.normal(0, 0.03), rotation_center=centre[i]) for i in range(n)]
    out = dict(input=name, pairs=n, mean_n1=mean_n1, mean_n2=mean_n2, estimates={})
    y0, t0 = errors(np.stack(inits), truth, centre)
    out["init_yaw_deg_median"], out["init_translation_m_median"] = float(np.median(y0)), float(np.median(t0))
    call = {"point": lambda c: eng.icp_refine_rows(rows, inits, 0.1, a.its, constrained=c),
            "plane": lambda c: eng.icp_plane_refine_rows(rows, inits, 0.1, a.normal_radius, a.its, constrained=c),
            "generalized": lambda c: eng.icp_generalized_refine_rows(rows, inits, 0.1, a.normal_radius, a.its, constrained=c)}
    for constrained in (True, False):
        for key in KEYS:
            call[key](constrained)
        ts, res = {key: [] for key in KEYS}, {}
        for _ in range(5):
            for key in KEYS:
                t = time.perf_counter(); res[key] = call[key](constrained); ts[key].append(time.perf_counter() - t)
        kms = {}
        for key in ("plane", "generalized"):
            eng.profile_enable(True); eng.profile_read(reset=True)
            call[key](constrained); eng.synchronize()
            kern = eng.profile_kernels(); eng.profile_read(reset=True); eng.profile_enable(False)
            kms[key] = {k: kern.get(k, (0.0, 0))[0] for k in TIMERS[key]}
        kind = "z-constrained" if constrained else "full rotation"
        e, tr_of = {}, {}
        for key in KEYS:
            yaw, tr = errors(res[key]["transforms"], truth, centre)
            it = res[key]["iterations"]
            e[key] = dict(stats(ts[key]), mean_iterations=float(it.mean()), share_at_limit=float((it >= a.its).mean()), mean_fitness=float(res[key]["fitness"].mean()),
                          yaw_deg_median=float(np.median(yaw)), yaw_deg_p90=float(np.percentile(yaw, 90)), translation_m_median=float(np.median(tr)),
                          translation_m_p90=float(np.percentile(tr, 90)), translation_m_max=float(tr.max()),
                          ms_per_evaluation=1e3 * float(np.median(ts[key])) / float(it.mean() + 1))
            tr_of[key] = tr
        rec = dict(e)
        for key, base in (("plane", "point"), ("generalized", "point"), ("generalized", "plane")):
            worse = np.flatnonzero(tr_of[key] > tr_of[base])
            rec["%s_worse_than_%s" % (key, base)] = dict(pairs=int(worse.size), share=float(worse.size) / n,
                                                          by_m_max=float((tr_of[key] - tr_of[base])[worse].max()) if worse.size else 0.0)
        for key in ("plane", "generalized"):
            rec[key + "_kernel_ms"] = kms[key]
            rec[key + "_over_point_time"] = e[key]["median_ms"] / e["point"]["median_ms"]
        out["estimates"][kind] = rec
        for key in KEYS:
            s = e[key]
            print("%-18s %-13s %-11s %3d pairs, n2 %7.0f: %8.2f ms (%.2f .. %.2f), mean iterations %5.2f, at the limit %5.1f %%, fitness %.3f, yaw error %.4f deg "
                  "(p90 %.4f), translation error %.2f mm (p90 %.2f, max %.1f)"
                  % (name, kind, key, n, mean_n2, s["median_ms"], s["min_ms"], s["max_ms"], s["mean_iterations"], 100 * s["share_at_limit"], s["mean_fitness"],
                     s["yaw_deg_median"], s["yaw_deg_p90"], 1e3 * s["translation_m_median"], 1e3 * s["translation_m_p90"], 1e3 * s["translation_m_max"]), flush=True)
        g = kms["generalized"]
        print("%-18s %-13s generalized / point time %.2f, plane / point %.2f; generalized kernels (device timers, one call): grid builds %.3f ms, normals stage "
              "(both clouds) %.3f ms, iterations %.3f ms; plane's normals stage %.3f ms; farther from the truth than point: plane %d, generalized %d of %d pairs; "
              "generalized farther than plane: %d"
              % (name, kind, rec["generalized_over_point_time"], rec["plane_over_point_time"], g["icp_grid_build"], g["icp_generalized_normals"], g["icp_generalized"],
                 kms["plane"]["icp_plane_normals"], rec["plane_worse_than_point"]["pairs"], rec["generalized_worse_than_point"]["pairs"], n,
                 rec["generalized_worse_than_plane"]["pairs"]), flush=True)
    return out


results = []
n, P = a.pairs, 1500
d = R.synth_pairs(n, P, dtype=np.float32)
off = np.zeros((n + 1, 2), np.int64); off[1:, 0] = off[1:, 1] = np.arange(1, n + 1) * P
eng.upload_dataset(d["pcs1"].reshape(-1, 3), d["pcs2"].reshape(-1, 3), off, np.zeros((n, 12), np.float32))
results.append(measure("synth_pairs 1500", n, P, P, d["translations"].astype(np.float64), d["rel_angles"][:, 0].astype(np.float64), d["pc1_centers"].astype(np.float64)))
for dist in [float(x) for x in a.distances.split(",")]:
    sc = [scenes.draw_scene(1000 + i, kind="cars", polar_dist_range=(dist, dist)) for i in range(n)]
    off = scenes.generate(eng, sc, seed=0, install=True)
    cnt = np.diff(off, axis=0)
    lab = np.stack([scenes.scene_labels(s) for s in sc]).astype(np.float64)
    results.append(measure("scene at %.1f m" % dist, n, float(cnt[:, 0].mean()), float(cnt[:, 1].mean()), lab[:, 0:3], lab[:, 3], lab[:, 4:7]))
    results[-1]["distance_m"] = dist
summary = dict(radius=0.1, normal_radius=a.normal_radius, iterations=a.its, point="icp_refine_rows with icp_search 1 (grid)", plane="icp_plane_refine_rows",
               generalized="icp_generalized_refine_rows",
               timing="wall time of one call (inits up, kernels, results down, stream synchronised), the three calls timed alternately after a warm-up of each; median of 5",
               results=results)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
json.dump(summary, open(a.out, "w"), indent=1)
eng.close()
