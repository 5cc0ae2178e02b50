# GPU: fast global registration throughput (alignnet_fgr_register_dataset: FPFH + FGR, the o3_gicp_fast baseline) on exactly the input of
# tools/global_reg_rate.py: 256 pairs x 1500-point clouds, Open3D's option values, median of 5 after a warm-up (host clock around calls that
# end in a stream synchronise), for both estimate kinds and both decrease_mu values.  Beside it, in the same process, the yardsticks: the
# RANSAC call (alignnet_global_register_dataset at 4,000,000 / 500) and the same call with max_validation = 0, which is the front end FGR
# shares (downsample .. forward matches, plus the RANSAC call's grid stage); FGR is reported as that front end + its tail.  Then one pair
# with a large target, and the NumPy restatement's time on a few pairs for context.  What the tail is made of comes from a run of its own:
#   rocprofv3 --kernel-trace --stats -d prof_out -- python tools/fgr_rate.py --fgr-only
import os, sys, time, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
import alignnet3d
from tests import global_reg_ref as G
from tests import fgr_ref as R
fgr_only = "--fgr-only" in sys.argv
n, P = 256, 1500
src, dst, truth = G.car_pairs(n, seed=1, n_points=P, scale=0.3, max_shift=0.3)
off = np.zeros((n + 1, 2), np.int64); off[1:, 0] = np.cumsum([len(s) for s in src]); off[1:, 1] = np.cumsum([len(t) for t in dst])
eng = alignnet3d.Engine()
eng.upload_dataset(np.concatenate(src), np.concatenate(dst), off, np.zeros((n, 12), np.float32))
rows = np.arange(n)


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); res = fn(); ts.append(time.perf_counter() - t)
    return float(np.median(ts)), res


one = eng.debug_fgr_stages(src[0], dst[0])
print("clouds: %d pairs, source %d / target %d points (70 %% subset), downsampled to about %d / %d, %d mutual matches" % (
    n, len(src[0]), len(dst[0]), one["counts"][0], one["counts"][1], len(one["cross"])))
for constrained in (True, False):
    kind = "z-constrained" if constrained else "full rotation"
    front = None
    if not fgr_only:
        front, _ = timed(lambda: eng.global_register_rows(rows, constrained=constrained, max_validation=0))
        ransac, _ = timed(lambda: eng.global_register_rows(rows, constrained=constrained))
        print("GPU %s, yardsticks: RANSAC call %.1f ms, its front end (max_validation = 0) %.1f ms" % (kind, ransac * 1e3, front * 1e3))
    for dm in (False, True):
        full, res = timed(lambda: eng.fgr_register_rows(rows, constrained=constrained, decrease_mu=dm))
        err = [abs(np.arctan2(E[1, 0], E[0, 0])) for E in (np.linalg.inv(truth[i]) @ res["transforms"][i] for i in range(n))]
        print("GPU %s, decrease_mu %s: %d pairs in %.1f ms (median of 5) = %.0f pairs/s%s (correspondences mean %.0f, min %d; trials mean %.0f, max %d; "
              "mean fitness at 2.5 cm %.3f; yaw within 0.05 rad of the truth for %d pairs)" % (
                  kind, dm, n, full * 1e3, n / full, "" if front is None else ": front end %.1f ms + tail %.1f ms" % (front * 1e3, (full - front) * 1e3),
                  res["correspondences"].mean(), res["correspondences"].min(), res["trials"].mean(), res["trials"].max(), res["fitness"].mean(),
                  int(np.sum(np.array(err) < 0.05))))
    if not fgr_only:
        none, _ = timed(lambda: eng.fgr_register_rows(rows, constrained=constrained, iteration_number=0))
        print("GPU %s, iteration_number = 0 (everything but the Gauss-Newton loop): %.1f ms" % (kind, none * 1e3))
if not fgr_only:
    for npts in (9000, 16000):
        s, d, _ = G.car_pairs(1, seed=31, n_points=npts, scale=0.9, max_shift=0.3)
        dt, res = timed(lambda: eng.fgr_register(s, d), reps=3)
        front, _ = timed(lambda: eng.global_register(s, d, max_validation=0), reps=3)
        cnt = eng.debug_fgr_stages(s[0], d[0])["counts"]
        print("GPU one pair, %d / %d downsampled points: %.1f ms, RANSAC call's front end %.1f ms (%d correspondences in %d trials, fitness %.3f)" % (
            cnt[0], cnt[1], dt * 1e3, front * 1e3, res["correspondences"][0], res["trials"][0], res["fitness"][0]))
eng.close()
if not fgr_only:
    t = time.perf_counter()
    for i in range(3): R.fgr_register(src[i], dst[i], stream=i)
    print("NumPy / SciPy restatement (context only): %.2f s per pair" % ((time.perf_counter() - t) / 3))
