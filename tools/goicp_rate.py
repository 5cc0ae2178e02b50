# GPU: Go-ICP registration (alignnet_goicp_register_dataset: branch-and-bound over yaw and translation) on tools/icp_rate.py's input,
# 256 pairs x 1500-point clouds, whole calls at Engine.GOICP_DEFAULTS, median of 5 with min and max after a warm-up, timed alternately
# with the RANSAC call (alignnet_global_register_dataset) in the same process.  Writes profiles/goicp_rate.json: ms per call, nodes per
# pair by level, the share of pairs per stop status, the gap error - lower_bound, the yaw error against the truth (and, the boxes being
# their own mirror image under a half turn, modulo pi) beside point-to-point ICP from the centroid start, the node kernel's registers /
# scratch / LDS from the build's remarks, the fp64 MFMA rate of one evaluation launch of 2^18 nodes through the debug hook (a host clock
# around upload + launch + read-back: a lower bound of the kernel's own rate) against the public fp64 matrix peak, and the NumPy
# restatement's seconds per pair at a reduced node budget.
import argparse, json, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
import alignnet3d
from oracle import alignnet_ref as R
from tests import goicp_ref as G

FP64_MATRIX_PEAK = 78.6e12   # MI355X data sheet, fp64 matrix (and vector) FLOP/s
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
flags = ap.parse_args()
REPS = flags.reps
n, P = flags.pairs, 1500
say = lambda *a: print(*a, flush=True)
d = R.synth_pairs(n, P, dtype=np.float32)
off = np.zeros((n + 1, 2), np.int64); off[1:, 0] = off[1:, 1] = np.arange(1, n + 1) * P
eng = alignnet3d.Engine()
eng.upload_dataset(d["pcs1"].reshape(-1, 3), d["pcs2"].reshape(-1, 3), off, np.zeros((n, 12), np.float32))
rows = np.arange(n)
truth = d["rel_angles"][:, 0].astype(np.float64)
wrap = lambda a, m: (a + m / 2) % m - m / 2


def stats(ts):
    return dict(median_ms=float(np.median(ts)) * 1e3, min_ms=float(np.min(ts)) * 1e3, max_ms=float(np.max(ts)) * 1e3, calls=len(ts))


def yaw_errors(T):
    yaw = np.arctan2(T[:, 1, 0], T[:, 0, 0])
    e, e_pi = np.abs(wrap(yaw - truth, 2 * np.pi)), np.abs(wrap(yaw - truth, np.pi))
    return dict(median_deg=float(np.rad2deg(np.median(e))), within_2deg=float(np.mean(e < np.deg2rad(2))),
                median_deg_mod_pi=float(np.rad2deg(np.median(e_pi))), within_2deg_mod_pi=float(np.mean(e_pi < np.deg2rad(2))))


go = lambda: eng.goicp_register_rows(rows)
ransac = lambda: eng.global_register_rows(rows)
t = time.perf_counter(); res = go(); warm = time.perf_counter() - t
say("warm-up call: %.2f s" % warm)
ransac()
reps = REPS if warm < 40.0 else 1   # (a call of most of a minute: one timed call, said so in the file)
tg, tr = [], []
for _ in range(reps):   # alternately, in one process
    t = time.perf_counter(); res = go(); tg.append(time.perf_counter() - t)
    t = time.perf_counter(); rr = ransac(); tr.append(time.perf_counter() - t)
    say("goicp %.1f ms, ransac %.1f ms" % (tg[-1] * 1e3, tr[-1] * 1e3))
status = {name: float(np.mean(res["status"] == k)) for k, name in enumerate(eng.GOICP_STATUS)}
gap = res["error"] - res["lower_bound"]
ev = res["evaluated"].astype(np.float64)
levels = int(np.max(np.nonzero(ev.sum(0))[0])) + 1 if ev.sum() else 0
init = eng.centroid_inits(d["pcs1"].reshape(-1, 3), d["pcs2"].reshape(-1, 3), off, rows)
p2p = eng.icp_refine_rows(rows, init, 0.1, 30)
refined = eng.goicp_register_rows(rows, refine="p2p")
say("refined call done")

# one evaluation launch: 2^18 nodes of pair 0 at the deepest level of the defaults, |S| = 256, |Q| = 1500
K = 1 << 18
depth = [8, 7, 7, 4]
rng = np.random.RandomState(0)
coords = np.stack([rng.randint(0, 1 << k, K) for k in depth], 1)
s0, t0 = d["pcs1"][0], d["pcs2"][0]
eng.debug_goicp_nodes(s0, t0, depth, coords)
te = []
for _ in range(5):
    t = time.perf_counter(); eng.debug_goicp_nodes(s0, t0, depth, coords); te.append(time.perf_counter() - t)
ns, nq = min(P, eng.GOICP_DEFAULTS["max_source"]), min(P, eng.GOICP_DEFAULTS["max_target"])
mfma = K * ((ns + 15) // 16) * ((nq + 15) // 16)
flops = mfma * 16 * 16 * 4 * 2
eval_s = float(np.median(te))

kernel = None
remarks = os.path.join(ROOT, "alignnet-3d_amd", "csrc", "alignnet_goicp.remarks")
if os.path.exists(remarks):
    m = re.search(r"Function Name: \S*goicp_eval_kernel\S*.*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)",
                  open(remarks).read(), re.S)
    if m:
        kernel = dict(vgprs=int(m.group(1)), agprs=int(m.group(2)), scratch_bytes_per_lane=int(m.group(3)), occupancy_waves_per_simd=int(m.group(4)),
                      lds_bytes_dynamic=32 * min(2048, (nq + 15) // 16 * 16))
eng.close()

# the restatement, at a node budget it can walk in NumPy (the defaults' frontier is the GPU's business)
small = G.params(max_frontier=1 << 10, starts=0)
t = time.perf_counter(); rs = G.search(s0, t0, small); ref_s = time.perf_counter() - t

out = dict(
    input="oracle.alignnet_ref.synth_pairs(%d, %d): boxes 4.5 x 1.8 x 1.5 m, yaw U(-pi/2, pi/2), shift <= 1 m; a box is its own image under a half turn" % (n, P),
    params={k: (list(v) if isinstance(v, tuple) else v) for k, v in eng.GOICP_DEFAULTS.items()},
    goicp=stats(tg), ransac=stats(tr), warmup_call_s=warm, pairs=n,
    nodes_evaluated_per_pair_by_level=[float(x) for x in ev.mean(0)[:levels]],
    nodes_surviving_per_pair_by_level=[float(x) for x in res["survived"].mean(0)[:levels]],
    nodes_evaluated_per_pair=float(ev.sum(1).mean()),
    status_share=status,
    gap=dict(median=float(np.median(gap)), max=float(np.max(gap)), error_median=float(np.median(res["error"])), eps=1e-4 * ns),
    fitness_mean=float(res["fitness"].mean()),
    yaw_error_goicp=yaw_errors(res["transforms"]), yaw_error_goicp_refined=yaw_errors(refined["transforms"]),
    yaw_error_p2point_centroid=yaw_errors(p2p["transforms"]), yaw_error_ransac=yaw_errors(rr["transforms"]),
    node_kernel=kernel,
    evaluation_launch=dict(nodes=K, source=ns, target=nq, seconds_median_of_5=eval_s, nodes_per_s=K / eval_s, mfma_count=mfma,
                           fp64_flop_per_s=flops / eval_s, share_of_fp64_matrix_peak=flops / eval_s / FP64_MATRIX_PEAK,
                           note="host clock around upload + launch + read-back of one debug call: a lower bound of the kernel's rate"),
    whole_call_fp64_flop_per_s=float(ev.sum() * ((ns + 15) // 16) * ((nq + 15) // 16) * 2048 / np.median(tg)),
    restatement=dict(seconds_per_pair=ref_s, max_frontier=1 << 10, starts=0, status=G.STATUS_NAMES[rs["status"]], nodes=int(rs["evaluated"].sum())))
json.dump(out, open(os.path.join(ROOT, "profiles", "goicp_rate.json"), "w"), indent=1)
print(json.dumps(out, indent=1))
