#!/usr/bin/env python3
"""GPU: the KITTI tracklet extraction (Engine.tracklet_upload_scans / tracklet_extract, csrc/alignnet_crop.hip) at the size of a KITTI tracking
sequence: 64 frames x 120,000 points (stride 4, as a .bin), 8 tracked boxes per frame, pairs between consecutive frames (504 pairs = 1,008 crop
jobs).  The frames are synthetic (ground returns over +- 60 m plus a cluster of returns on every object; under 2 % of a frame's points are in any
box).  Before timing, two pairs of the timed call are compared with the restatement (tests/tracklet_ref.py): offsets and points, bit for bit.
Reported, upload and extract separately: wall time of the whole call (the stream is synchronised inside it), median of 5 with min .. max; the two
stage timers ("tracklet_test" = membership + counts, "tracklet_compact" = scan + scatter; HIP events, median of 3); the bytes of scan the test stage
reads per second against the measured copy peak of the chip (6.29 TB/s); a sweep of the points per frame (the base frame tiled), which shows
where the stage timers start to grow with the size, i.e. where the call stops being bound by launches and the host; VGPRs, scratch and LDS of
the kernels from the build remarks.  Beside it, on the host of the same machine: the NumPy restatement and the reference's method (scipy's
Delaunay on the box corners, find_simplex on the whole frame) per pair, median over 8 pairs.  Writes profiles/tracklet_rate.json; --markdown FILE
prints the README row from such a file.
Usage: python tools/tracklet_rate.py [--frames 64] [--points 120000] [--boxes 8] [--out FILE] | --markdown FILE"""
import argparse, json, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(ROOT, 'alignnet-3d_amd')); sys.path.insert(0, ROOT)
COPY_PEAK = 6.29e12   # bytes per second, the chip's measured copy peak
STAGES = ("tracklet_test", "tracklet_compact")


def make_frames(F, n, nbox, seed=0):
    """F frames of n points [n, 4] and nbox tracks: boxes [F, nbox, 7], moving a little from frame to frame."""
    g = np.random.RandomState(seed)
    box = np.stack([g.uniform(-25, 25, nbox), g.uniform(1.4, 1.9, nbox), g.uniform(5, 55, nbox), g.uniform(1.4, 1.9, nbox), g.uniform(1.5, 1.9, nbox),
                    g.uniform(3.5, 4.6, nbox), g.uniform(-np.pi, np.pi, nbox)], 1)
    frames, boxes = [], []
    per_obj = max(1, n // 250)   # 0.4 % of the frame around every object; about half of them inside its box
    for _ in range(F):
        box = box + np.concatenate([g.uniform(-0.5, 0.5, (nbox, 3)), np.zeros((nbox, 3)), g.uniform(-0.05, 0.05, (nbox, 1))], 1)
        pts = np.empty((n, 4), np.float32)
        pts[:, 0], pts[:, 1] = g.uniform(-60, 60, n), g.uniform(-60, 60, n)
        pts[:, 2], pts[:, 3] = g.normal(-1.7, 0.05, n), g.uniform(0, 1, n)
        for k, b in enumerate(box):
            cam = b[:3] - [0, b[3] / 2, 0] + g.uniform(-1, 1, (per_obj, 3)) * [2.6, 1.0, 2.6]
            pts[k * per_obj:(k + 1) * per_obj, :3] = np.stack([cam[:, 2], -cam[:, 0], -cam[:, 1]], 1)
        frames.append(pts[g.permutation(n)])
        boxes.append(box.copy())
    return frames, np.array(boxes)


def pair_args(F, boxes):
    from alignnet3d import tracklets as T
    fr, bx, dz = [], [], []
    for f in range(F - 1):
        for k in range(boxes.shape[1]):
            fr.append([f, f + 1]); bx.append([boxes[f, k], boxes[f + 1, k]]); dz.append([0.0, np.float32(T.labels12(boxes[f, k], boxes[f + 1, k])[1])])
    return np.array(fr, np.int32), np.array(bx), np.array(dz, np.float32)


def resources():
    path = os.path.join(ROOT, "alignnet-3d_amd", "csrc", "alignnet_crop.remarks")
    if not os.path.exists(path):
        return None
    out, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((k for k in ("crop_test_kernelINS_7BoxCropELi4", "crop_test_kernelINS_7BoxCropELi3", "tracklet_scan_kernel",
                                     "crop_scatter_kernelINS_7BoxCropELi4", "crop_scatter_kernelINS_7BoxCropELi3") if k in m.group(1)), None)
            if name:
                out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def med(x):
    return dict(ms=1e3 * float(np.median(x)), ms_min=1e3 * min(x), ms_max=1e3 * max(x))


def run(a):
    import alignnet3d
    from tests import tracklet_ref as R
    from alignnet3d import tracklets as T
    frames, boxes = make_frames(a.frames, a.points, a.boxes)
    fr, bx, dz = pair_args(a.frames, boxes)
    eng = alignnet3d.Engine()
    eng.tracklet_upload_scans(frames)
    off = eng.tracklet_extract(fr, bx, dz)
    p1, p2 = eng.tracklet_read(off)
    for b in (0, len(fr) - 1):   # two pairs of the timed call against the restatement
        ro, r1, r2 = R.extract(frames, fr[b:b + 1], bx[b:b + 1], dz[b:b + 1])
        assert np.array_equal(ro[1], off[b + 1] - off[b]), "pair %d: offsets differ from the restatement's" % b
        assert np.array_equal(p1[off[b, 0]:off[b + 1, 0]].view(np.uint32), r1.view(np.uint32)) and np.array_equal(p2[off[b, 1]:off[b + 1, 1]].view(np.uint32), r2.view(np.uint32)), b
    in_box = float(np.mean([np.logical_or.reduce([R.inside(frames[f], b) for b in boxes[f]]).mean() for f in (0, a.frames - 1)]))
    t_up, t_ex = [], []
    for _ in range(5):
        t = time.perf_counter(); eng.tracklet_upload_scans(frames); t_up.append(time.perf_counter() - t)
        t = time.perf_counter(); eng.tracklet_extract(fr, bx, dz); t_ex.append(time.perf_counter() - t)
    cat = np.ascontiguousarray(np.concatenate(frames, 0))
    offs = np.arange(a.frames + 1, dtype=np.int64) * a.points
    t_up_cat = []
    for _ in range(5):
        t = time.perf_counter(); eng.tracklet_upload_scans((cat, offs)); t_up_cat.append(time.perf_counter() - t)

    def stages(reps=3):
        eng.profile_enable(True); eng.profile_read(reset=True)
        acc = {k: [] for k in STAGES}
        for _ in range(reps):
            eng.tracklet_extract(fr, bx, dz); kern = eng.profile_kernels(); eng.profile_read(reset=True)
            for k in STAGES: acc[k].append(kern.get(k, (0.0, 0))[0])
        eng.profile_enable(False)
        return {k: float(np.median(v)) for k, v in acc.items()}

    st = stages()
    scan_bytes = a.frames * a.points * 16
    sweep = []
    for mult in (1, 4, 16):
        if mult > 1:
            eng.tracklet_upload_scans((np.ascontiguousarray(np.tile(cat.reshape(a.frames, a.points, 4), (1, mult, 1)).reshape(-1, 4)), offs * mult))
            eng.tracklet_extract(fr, bx, dz)
        s = stages()
        t = []
        for _ in range(3):
            t0 = time.perf_counter(); eng.tracklet_extract(fr, bx, dz); t.append(time.perf_counter() - t0)
        sweep.append(dict(points_per_frame=a.points * mult, scan_bytes=scan_bytes * mult, test_ms=s["tracklet_test"], compact_ms=s["tracklet_compact"],
                          extract_ms=1e3 * float(np.median(t)), test_bytes_per_s=scan_bytes * mult / (1e-3 * s["tracklet_test"]) if s["tracklet_test"] > 0 else None))
    eng.close()
    # the host of the same machine, per pair
    from scipy.spatial import Delaunay
    t_np, t_hull = [], []
    camera = lambda s: np.stack([-s[:, 1], -s[:, 2], s[:, 0]], 1).astype(np.float64)
    for b in range(0, len(fr), max(1, len(fr) // 8))[:8]:
        t = time.perf_counter()
        for k in range(2): R.crop(frames[fr[b, k]], bx[b, k], dz[b, k])
        t_np.append(time.perf_counter() - t)
        t = time.perf_counter()
        for k in range(2):
            s = frames[fr[b, k]]
            s[Delaunay(T.box_corners(bx[b, k])).find_simplex(camera(s)) >= 0]
        t_hull.append(time.perf_counter() - t)
    res = dict(frames=a.frames, points_per_frame=a.points, boxes_per_frame=a.boxes, pairs=int(len(fr)), jobs=int(2 * len(fr)), stride=4, scan_bytes=scan_bytes,
               points_in_a_box_fraction=in_box, crop_points=[int(off[-1, 0]), int(off[-1, 1])], chunk=eng_opts["chunk"], jobs_per_pass=eng_opts["jobs_per_pass"],
               upload_list=med(t_up), upload_concatenated=med(t_up_cat), extract=med(t_ex), stage_ms=st,
               test_bytes_per_s=scan_bytes / (1e-3 * st["tracklet_test"]), test_share_of_copy_peak=scan_bytes / (1e-3 * st["tracklet_test"]) / COPY_PEAK,
               extract_ms_per_pair=1e3 * float(np.median(t_ex)) / len(fr), sweep=sweep, kernel_resources=resources(),
               host_numpy_restatement_ms_per_pair=1e3 * float(np.median(t_np)), host_scipy_delaunay_ms_per_pair=1e3 * float(np.median(t_hull)))
    return res


eng_opts = {}


def markdown(path):
    d = json.load(open(path))["result"]
    print("| KITTI tracklet extraction, %d frames x %s points, %d pairs (`tools/tracklet_rate.py`) | upload %.1f ms (%.1f .. %.1f), extract %.2f ms (%.2f .. %.2f) = %.1f us per pair; "
          "stages: test %.3f ms (%.2f TB/s of scan read, %.0f %% of the 6.29 TB/s copy peak), compact %.3f ms; host, per pair: NumPy restatement %.1f ms, scipy Delaunay %.1f ms |" %
          (d["frames"], format(d["points_per_frame"], ","), d["pairs"], d["upload_concatenated"]["ms"], d["upload_concatenated"]["ms_min"], d["upload_concatenated"]["ms_max"],
           d["extract"]["ms"], d["extract"]["ms_min"], d["extract"]["ms_max"], 1e3 * d["extract_ms_per_pair"], d["stage_ms"]["tracklet_test"], d["test_bytes_per_s"] / 1e12,
           100 * d["test_share_of_copy_peak"], d["stage_ms"]["tracklet_compact"], d["host_numpy_restatement_ms_per_pair"], d["host_scipy_delaunay_ms_per_pair"]))
    for s in d["sweep"]:
        print("  %9d points per frame: extract %.2f ms, test %.3f ms (%.2f TB/s), compact %.3f ms" %
              (s["points_per_frame"], s["extract_ms"], s["test_ms"], (s["test_bytes_per_s"] or 0) / 1e12, s["compact_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracklet_rate.json"))
    ap.add_argument("--markdown", metavar="FILE", help="print the README row from a result file; nothing is run")
    a = ap.parse_args()
    if a.markdown:
        return markdown(a.markdown)
    import alignnet3d
    e = alignnet3d.Engine()
    eng_opts.update(chunk=e.get_option("tracklet_chunk"), jobs_per_pass=e.get_option("tracklet_jobs_per_pass"))
    e.close()
    commit = open(os.path.join(ROOT, ".build_commit")).read().strip() if os.path.exists(os.path.join(ROOT, ".build_commit")) else None
    summary = dict(tool="tracklet_rate", commit=commit,
                   timing="wall time of one whole call (tracklet_upload_scans of a list of frames, of one concatenated array, tracklet_extract: tables up, three kernels, "
                          "the offsets copy, stream synchronised), median of 5 after a warm-up; stage_ms = HIP-event time of the stages, median of 3 calls; "
                          "test_bytes_per_s = bytes of scan (16 per point) over the test stage's time; sweep = the base frames tiled 1, 4, 16 times (same boxes); host "
                          "figures = median over 8 pairs of both crops of a pair on the CPU of the same machine",
                   result=run(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(summary, open(a.out, "w"), indent=1)
    markdown(a.out)


if __name__ == "__main__":
    main()
