# GPU: whole-call wall clock of the one-call registration (Engine.register_rows) against the composition of the calls it joins
# (forward_rows + host decode + get_mat_angle + icp_refine_rows), on tools/icp_rate.py's input: 256 pairs x 1500 points, SynthCars widths, N = 1024,
# z-constrained estimate.  The two paths alternate in one process; per (B, its) the median of 5 whole calls with min and max.
#   python tools/register_rate.py [--out profiles/register_rate.json]
#   python tools/register_rate.py --calls K [--B 8] [--its 30]   # warm up, then K register_rows calls and nothing else (for an API / kernel trace)
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
import alignnet3d
import evaluation
from oracle import alignnet_ref as R

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--calls", type=int, default=-1)
ap.add_argument("--B", type=int, default=8)
ap.add_argument("--its", type=int, default=30)
args = ap.parse_args()

n, P = 256, 1500
d = R.synth_pairs(n, P, dtype=np.float32)
off = np.zeros((n + 1, 2), np.int64); off[1:, 0] = off[1:, 1] = np.arange(1, n + 1) * P
eng = alignnet3d.Engine()
nb = eng.num_bins
eng.upload_dataset(d["pcs1"].reshape(-1, 3), d["pcs2"].reshape(-1, 3), off, np.zeros((n, 12), np.float32))
SEED, K = 11, 2 * np.pi / nb


def decode(logits):   # models/tp8.py:55-65 as the evaluation loop runs it: a list comprehension per logit set
    classes = np.argmax(logits[:, :nb], axis=1)
    out = []
    for c, r in zip(classes, logits[:, nb:]):
        a = c * K + r[c]
        out.append(a - 2 * np.pi if a > np.pi else a)
    return np.array(out)


def composition(rows, its):   # only calls that exist without the one-call registration
    ep = eng.forward_rows(rows, SEED)
    a1, a2, ar = decode(ep["pred_pc1angle_logits"]), decode(ep["pred_pc2angle_logits"]), decode(ep["pred_remaining_angle_logits"])
    pa = a2 - a1 + ar
    inits = [evaluation.get_mat_angle(ep["pred_translations"][i], pa[i], rotation_center=ep["pred_s2_pc1centers"][i]) for i in range(len(rows))]
    return eng.icp_refine_rows(rows, inits, 0.1, its)["transforms"]


def single(rows, its):
    return eng.register_rows(rows, SEED, refine="point", radius=0.1, its=its)["transforms"]


if args.calls >= 0:
    rows = np.arange(args.B)
    for _ in range(3):
        single(rows, args.its)
    for _ in range(args.calls):
        single(rows, args.its)
    print("register_rows: 3 warm-up calls + %d calls, B = %d, its = %d" % (args.calls, args.B, args.its))
    sys.exit(0)

result = {"input": "%d pairs x %d points, default (SynthCars) widths, N = %d, radius 0.1, z-constrained, random initial weights" % (n, P, eng.num_points),
          "method": "whole calls, wall clock, the two paths alternating in one process; median of 5 with min and max, milliseconds", "cases": []}
for B in (1, 8, 256):
    rows = np.arange(B)
    for its in (0, 30):
        a, b = composition(rows, its), single(rows, its)   # warm-up (workspaces grow here), and the two paths agree
        agree = float(np.abs(a - b).max())
        t = {"composition": [], "register_rows": []}
        for _ in range(5):
            for name, fn in (("composition", composition), ("register_rows", single)):
                t0 = time.perf_counter(); fn(rows, its); t[name].append((time.perf_counter() - t0) * 1e3)
        case = {"B": B, "its": its, "max_abs_difference_of_transforms": agree}
        for name, v in t.items():
            case[name + "_ms"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
        case["speedup_median"] = case["composition_ms"]["median"] / case["register_rows_ms"]["median"]
        result["cases"].append(case)
        print("B = %3d its = %2d: composition %.3f ms (%.3f .. %.3f), register_rows %.3f ms (%.3f .. %.3f), x%.2f; transforms differ by %.1e" % (
            B, its, case["composition_ms"]["median"], case["composition_ms"]["min"], case["composition_ms"]["max"], case["register_rows_ms"]["median"],
            case["register_rows_ms"]["min"], case["register_rows_ms"]["max"], case["speedup_median"], agree))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
eng.close()
