#!/usr/bin/env python3
"""GPU: the image-frustum crop (Engine.tracklet_extract_frustum, csrc/alignnet_crop.hip) on the input of tools/tracklet_rate.py: 64 frames x
120,000 points (stride 4), 8 tracked boxes per frame, pairs between consecutive frames (504 pairs = 1,008 crop jobs); the rectangles are the
projected 3D boxes under a KITTI-like calibration (tests/frustum_cases.KITTI, image 1242 x 375).  Before timing, two pairs of the timed call
are compared with the restatement (tests/frustum_ref.py): offsets and points, bit for bit.  Then the frustum extraction and the box
extraction of the same scans are timed ALTERNATELY in one process: wall time of the whole call (the stream is synchronised inside it), median
of 5 with min .. max.  Also reported, for both: the two stage timers ("tracklet_test" = membership + counts, "tracklet_compact" = scan +
scatter; HIP events, median of 3), the points per crop, the bytes of scan the test stage reads per second against the measured copy peak of the
chip (6.29 TB/s); VGPRs, scratch and LDS of the frustum kernels from the build remarks; and the NumPy restatement's time per pair on the host
of the same machine, median over 8 pairs.  Writes profiles/frustum_rate.json; --markdown FILE prints the README row from such a file.
Usage: python tools/frustum_rate.py [--frames 64] [--points 120000] [--boxes 8] [--out FILE] | --markdown FILE"""
import argparse, json, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'alignnet-3d_amd'), ROOT):
    sys.path.insert(0, p)
from tracklet_rate import COPY_PEAK, STAGES, make_frames, med, pair_args  # noqa: E402
KERNELS = ("crop_test_kernelINS_11FrustumCropELi4", "crop_test_kernelINS_11FrustumCropELi3", "crop_scatter_kernelINS_11FrustumCropELi4",
           "crop_scatter_kernelINS_11FrustumCropELi3")


def resources():
    path = os.path.join(ROOT, "alignnet-3d_amd", "csrc", "alignnet_crop.remarks")
    if not os.path.exists(path):
        return None
    out, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((k for k in KERNELS if k in m.group(1)), None)
            if name:
                out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def run(a):
    import alignnet3d
    from alignnet3d import tracklets as T
    from tests import frustum_cases as C
    from tests import frustum_ref as R
    frames, boxes = make_frames(a.frames, a.points, a.boxes)
    fr, bx, dz = pair_args(a.frames, boxes)
    M, image = T.projection(C.KITTI), C.KITTI_IMAGE
    rects = np.array([[C.box_rect(b, M) for b in pair] for pair in bx])
    eng = alignnet3d.Engine()
    chunk, per_pass = eng.get_option("tracklet_chunk"), eng.get_option("tracklet_jobs_per_pass")
    eng.tracklet_upload_scans(frames)
    frustum = lambda: eng.tracklet_extract_frustum(fr, rects, M, image, dz)
    box = lambda: eng.tracklet_extract(fr, bx, dz)
    off = frustum()
    p1, p2 = eng.tracklet_read(off)
    for b in (0, len(fr) - 1):   # two pairs of the timed call against the restatement
        ro, r1, r2 = R.extract(frames, fr[b:b + 1], rects[b:b + 1], M, image, dz[b:b + 1])
        assert np.array_equal(ro[1], off[b + 1] - off[b]), "pair %d: offsets differ from the restatement's" % b
        assert np.array_equal(p1[off[b, 0]:off[b + 1, 0]].view(np.uint32), r1.view(np.uint32)) and np.array_equal(p2[off[b, 1]:off[b + 1, 1]].view(np.uint32), r2.view(np.uint32)), b
    off_box = box()
    t = {"frustum": [], "box": []}
    for _ in range(5):   # alternately, whole calls
        for name, call in (("frustum", frustum), ("box", box)):
            t0 = time.perf_counter(); call(); t[name].append(time.perf_counter() - t0)

    def stages(call, reps=3):
        eng.profile_enable(True); eng.profile_read(reset=True)
        acc = {k: [] for k in STAGES}
        for _ in range(reps):
            call(); kern = eng.profile_kernels(); eng.profile_read(reset=True)
            for k in STAGES: acc[k].append(kern.get(k, (0.0, 0))[0])
        eng.profile_enable(False)
        return {k: float(np.median(v)) for k, v in acc.items()}

    st = {"frustum": stages(frustum), "box": stages(box)}
    eng.close()
    t_np = []
    for b in range(0, len(fr), max(1, len(fr) // 8))[:8]:   # the host of the same machine, per pair
        t0 = time.perf_counter()
        for k in range(2): R.crop(frames[fr[b, k]], M, image, rects[b, k], dz[b, k])
        t_np.append(time.perf_counter() - t0)
    scan_bytes = a.frames * a.points * 16
    rate = lambda ms: scan_bytes / (1e-3 * ms) if ms > 0 else None
    share = lambda ms: scan_bytes / (1e-3 * ms) / COPY_PEAK if ms > 0 else None
    side = lambda name, o: dict(extract=med(t[name]), stage_ms=st[name], crop_points=[int(o[-1, 0]), int(o[-1, 1])], points_per_crop=float(o[-1].sum()) / (2 * len(fr)),
                                test_bytes_per_s=rate(st[name]["tracklet_test"]), test_share_of_copy_peak=share(st[name]["tracklet_test"]))
    return dict(frames=a.frames, points_per_frame=a.points, boxes_per_frame=a.boxes, pairs=int(len(fr)), jobs=int(2 * len(fr)), stride=4, scan_bytes=scan_bytes,
                image=list(image), clip=2.0, chunk=chunk, jobs_per_pass=per_pass, empty_crops=int((np.diff(off, axis=0) == 0).sum()), frustum=side("frustum", off),
                box=side("box", off_box), kernel_resources=resources(), host_numpy_restatement_ms_per_pair=1e3 * float(np.median(t_np)))


def markdown(path):
    d = json.load(open(path))["result"]
    f, b = d["frustum"], d["box"]
    print("| KITTI image-frustum crop (`from_bbox2d`), %d frames x %s points, %d pairs (`tools/frustum_rate.py`) | extract %.2f ms (%.2f .. %.2f), %.0f points per crop; "
          "the box extraction of the same scans in the same process, alternately: %.2f ms (%.2f .. %.2f), %.0f points per crop; stages, frustum / box: test %.3f / %.3f ms "
          "(%.2f / %.2f TB/s of scan read, %.0f / %.0f %% of the 6.29 TB/s copy peak), compact %.3f / %.3f ms; host, per pair: NumPy restatement %.1f ms |" %
          (d["frames"], format(d["points_per_frame"], ","), d["pairs"], f["extract"]["ms"], f["extract"]["ms_min"], f["extract"]["ms_max"], f["points_per_crop"],
           b["extract"]["ms"], b["extract"]["ms_min"], b["extract"]["ms_max"], b["points_per_crop"], f["stage_ms"]["tracklet_test"], b["stage_ms"]["tracklet_test"],
           (f["test_bytes_per_s"] or 0) / 1e12, (b["test_bytes_per_s"] or 0) / 1e12, 100 * (f["test_share_of_copy_peak"] or 0), 100 * (b["test_share_of_copy_peak"] or 0),
           f["stage_ms"]["tracklet_compact"], b["stage_ms"]["tracklet_compact"], d["host_numpy_restatement_ms_per_pair"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frustum_rate.json"))
    ap.add_argument("--markdown", metavar="FILE", help="print the README row from a result file; nothing is run")
    a = ap.parse_args()
    if a.markdown:
        return markdown(a.markdown)
    commit = open(os.path.join(ROOT, ".build_commit")).read().strip() if os.path.exists(os.path.join(ROOT, ".build_commit")) else None
    summary = dict(tool="frustum_rate", commit=commit,
                   timing="wall time of one whole call (tables up, three kernels, the offsets copy, stream synchronised) of tracklet_extract_frustum and of tracklet_extract "
                          "on the same uploaded scans, alternately in one process, median of 5 after a warm-up of each; stage_ms = HIP-event time of the stages, median of "
                          "3 calls; test_bytes_per_s = bytes of scan (16 per point) over the test stage's time; the host figure = median over 8 pairs of both crops of "
                          "a pair by tests/frustum_ref.py on the CPU of the same machine",
                   result=run(a))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(summary, open(a.out, "w"), indent=1)
    markdown(a.out)


if __name__ == "__main__":
    main()
