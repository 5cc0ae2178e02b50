# GPU: the evaluation call (Engine.evaluate_registration_rows: fitness, inlier RMSE and, on request, Open3D's information matrix of given
# transforms) against the call the project already had for the same two numbers, Engine.icp_refine_rows(..., its=0), at the same radius and
# transforms.  Inputs: tools/icp_rate.py's (256 pairs x 1,500 points, the scan) and one dense input of tools/icp_dense_rate.py (scenes at 11.8 m,
# about 6,000 target points, the grid search).  First the two calls' fitness and rmse are compared; then the three variants -- evaluate, evaluate
# with want_information, icp_refine its=0 -- are warmed up and timed alternately in this process: wall time of the whole call (transforms up,
# kernels, results down, the stream synchronised inside it), median of 5 with min .. max.  Writes profiles/reg_eval_rate.json.
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
import alignnet3d
from alignnet3d import scenes
from oracle import alignnet_ref as R
from oracle import icp_ref as I

p = argparse.ArgumentParser()
p.add_argument("--pairs", type=int, default=256)
p.add_argument("--pairs-dense", type=int, default=64)
p.add_argument("--distance", type=float, default=11.8, help="sensor distance (m) of the dense scenes")
p.add_argument("--radius", type=float, default=0.1)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "reg_eval_rate.json"))
a = p.parse_args()
eng = alignnet3d.Engine()
rng = np.random.default_rng(0)


def inits_of(trans, angle, centre):
    return [I.get_mat_angle(trans[i] + rng.normal(0, 0.05, 3), float(angle[i]) + rng.normal(0, 0.03), rotation_center=centre[i]) for i in range(len(trans))]


def measure(name, n, mean_n1, mean_n2, T, search):
    rows = np.arange(n)
    eng.set_option("icp_search", search)
    calls = {"evaluate": lambda: eng.evaluate_registration_rows(rows, T, threshold=a.radius),
             "evaluate_information": lambda: eng.evaluate_registration_rows(rows, T, threshold=a.radius, want_information=True),
             "icp_refine_its0": lambda: eng.icp_refine_rows(rows, T, radius=a.radius, its=0)}
    res = {k: f() for k, f in calls.items()}   # (the warm-up)
    same_fit = bool(np.array_equal(res["evaluate"]["fitness"], res["icp_refine_its0"]["fitness"]))
    rmse_gap = float(np.max(np.abs(res["evaluate"]["rmse"] - res["icp_refine_its0"]["rmse"]) / np.maximum(res["icp_refine_its0"]["rmse"], 1e-300)))
    assert same_fit and rmse_gap <= 1e-12, (name, same_fit, rmse_gap)
    assert np.array_equal(res["evaluate"]["rmse"], res["evaluate_information"]["rmse"])
    ts = {k: [] for k in calls}
    for _ in range(5):
        for k, f in calls.items():
            t = time.perf_counter(); f(); ts[k].append(1e3 * (time.perf_counter() - t))
    out = dict(input=name, pairs=n, mean_n1=mean_n1, mean_n2=mean_n2, search=("scan", "grid")[search], radius=a.radius, same_fitness=same_fit,
               worst_relative_rmse_gap=rmse_gap, rmse_bit_identical=bool(np.array_equal(res["evaluate"]["rmse"], res["icp_refine_its0"]["rmse"])),
               mean_fitness=float(res["evaluate"]["fitness"].mean()), ms={})
    for k, v in ts.items():
        out["ms"][k] = dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
    m = out["ms"]
    out["evaluate_over_icp_refine_its0"] = m["evaluate"]["median"] / m["icp_refine_its0"]["median"]
    out["information_over_evaluate"] = m["evaluate_information"]["median"] / m["evaluate"]["median"]
    spread = max(m["evaluate"]["max"] - m["evaluate"]["min"], m["evaluate_information"]["max"] - m["evaluate_information"]["min"])
    out["information_cost_exceeds_spread"] = bool(m["evaluate_information"]["median"] - m["evaluate"]["median"] > spread)
    print("%-18s %-4s %3d pairs, n2 %6.0f, fitness %.3f (equal to icp_refine its=0: %s, rmse gap %.2g): " % (name, out["search"], n, mean_n2, out["mean_fitness"], same_fit, rmse_gap)
          + ", ".join("%s %.3f ms (%.3f .. %.3f)" % (k, v["median"], v["min"], v["max"]) for k, v in m.items())
          + "; evaluate / icp_refine its=0 = %.3f, with information / without = %.3f (beyond the spread: %s)"
          % (out["evaluate_over_icp_refine_its0"], out["information_over_evaluate"], out["information_cost_exceeds_spread"]), flush=True)
    return out


results = []
n, P = a.pairs, 1500
d = R.synth_pairs(n, P, dtype=np.float32)
off = np.zeros((n + 1, 2), np.int64); off[1:, 0] = off[1:, 1] = np.arange(1, n + 1) * P
eng.upload_dataset(d["pcs1"].reshape(-1, 3), d["pcs2"].reshape(-1, 3), off, np.zeros((n, 12), np.float32))
results.append(measure("synth_pairs 1500", n, P, P, inits_of(d["translations"], d["rel_angles"][:, 0], d["pc1_centers"]), 0))
n = a.pairs_dense
sc = [scenes.draw_scene(1000 + i, kind="cars", polar_dist_range=(a.distance, a.distance)) for i in range(n)]
off = scenes.generate(eng, sc, seed=0, install=True)
cnt = np.diff(off, axis=0)
lab = np.stack([scenes.scene_labels(s) for s in sc]).astype(np.float64)
results.append(measure("scene at %.1f m" % a.distance, n, float(cnt[:, 0].mean()), float(cnt[:, 1].mean()), inits_of(lab[:, 0:3], lab[:, 3], lab[:, 4:7]), 1))
summary = dict(timing="wall time of one call (transforms up, kernels, results down, stream synchronised), the three variants timed alternately after a warm-up of each, "
                      "median of 5 with min and max", results=results)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
json.dump(summary, open(a.out, "w"), indent=1)
eng.close()
