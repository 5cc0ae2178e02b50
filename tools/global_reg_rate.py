# GPU: global registration throughput (alignnet_global_register_dataset: FPFH + RANSAC, the o3_gicp baseline), 256 pairs x 1500-point
# clouds at Open3D's defaults (4,000,000 iterations / 500 validations), median of 5 after a warm-up, for both estimate kinds; split into
# the front end (everything before the RANSAC loop: the same call with max_validation = 0) and the RANSAC loop (the difference).  Then
# the cost of one pair that never passes the pre-checks (all 4,000,000 iterations drawn), of a target above the LDS-resident size
# (validation grid read from HBM) next to one below it, and the NumPy restatement's time on a few pairs for context.
import os, sys, time, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
import alignnet3d
from tests import global_reg_ref as G
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


one = eng.debug_global_stages(src[0], dst[0])
print("clouds: %d pairs, source %d / target %d points (70 %% subset), downsampled to about %d / %d" % (n, len(src[0]), len(dst[0]), one["counts"][0], one["counts"][1]))
for constrained in (True, False):
    front, _ = timed(lambda: eng.global_register_rows(rows, constrained=constrained, max_validation=0))
    full, res = timed(lambda: eng.global_register_rows(rows, constrained=constrained))
    err = [abs(np.arctan2(E[1, 0], E[0, 0])) for E in (np.linalg.inv(truth[i]) @ res["transforms"][i] for i in range(n))]
    print("GPU %s: %d pairs in %.1f ms (median of 5) = %.0f pairs/s: front end %.1f ms, RANSAC %.1f ms (validations mean %.0f, min %d; iterations mean %.0f, "
          "max %d; mean fitness %.3f; yaw within 0.05 rad of the truth for %d pairs)" % (
              "z-constrained" if constrained else "full rotation", n, full * 1e3, n / full, front * 1e3, (full - front) * 1e3, res["validations"].mean(),
              res["validations"].min(), res["iterations"].mean(), res["iterations"].max(), res["fitness"].mean(), int(np.sum(np.array(err) < 0.05))))
# a pair that never passes: the target is the source at twice the size, so every edge-length check fails
never_s, never_t = [src[0]], [(src[0] * 2).astype(np.float32)]
for constrained in (True, False):
    dt, res = timed(lambda: eng.global_register(never_s, never_t, constrained=constrained), reps=3)
    print("GPU %s, one pair that never passes the pre-checks: %.1f ms for %d iterations (%d validations)" % (
        "z-constrained" if constrained else "full rotation", dt * 1e3, res["iterations"][0], res["validations"][0]))
# the validation grid in LDS and in HBM: targets below and above the LDS-resident size, 500 validations each
for npts in (9000, 16000):
    s, d, _ = G.car_pairs(1, seed=31, n_points=npts, scale=0.9, max_shift=0.3)
    front, _ = timed(lambda: eng.global_register(s, d, max_validation=0), reps=3)
    dt, res = timed(lambda: eng.global_register(s, d), reps=3)
    cnt = eng.debug_global_stages(s[0], d[0], max_validation=0)["counts"]
    print("GPU one pair, %d / %d downsampled points (%s): %.1f ms, front end %.1f ms, RANSAC %.1f ms for %d validations in %d iterations" % (
        cnt[0], cnt[1], "grid in LDS" if cnt[1] <= 6314 else "grid in HBM", dt * 1e3, front * 1e3, (dt - front) * 1e3, res["validations"][0], res["iterations"][0]))
eng.close()
t = time.perf_counter()
for i in range(3): G.global_register(src[i], dst[i], True, 0, i)
dc = (time.perf_counter() - t) / 3
print("NumPy / SciPy restatement (context only): %.2f s per pair" % dc)
