"""CPU: the host side of the image-frustum crop (alignnet3d/tracklets.py read_calib / projection / read_image_size, make_kitti_dataset.py's
parser, the C header) and its definition (tests/frustum_ref.py) against the reference's recorded outputs (tests/golden/frustum_vectors.*,
made by tests/golden/make_frustum_golden.py), and the five wrong kernels restated in NumPy that the GPU tests' inputs must refuse."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import alignnet3d
from alignnet3d import _capi
from alignnet3d import tracklets as T
from tests import frustum_cases as C
from tests import frustum_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CHUNK, PER_PASS = 1024, 32   # only size the cases here; the GPU tests read the engine's options


def _golden():
    return np.load(os.path.join(GOLD, "frustum_vectors.npz")), json.load(open(os.path.join(GOLD, "frustum_vectors.json")))


def _chain(calib, points):
    """project_velo_to_image as the reference evaluates it: three products, point by point (pointcloud.py:157-202)."""
    hom = lambda a: np.hstack((a, np.ones((len(a), 1))))
    ref = np.dot(hom(points), np.transpose(calib.V2C))
    rect = np.transpose(np.dot(calib.R0, np.transpose(ref)))
    px = np.dot(hom(rect), np.transpose(calib.P))
    with np.errstate(all="ignore"):
        return px[:, 0] / px[:, 2], px[:, 1] / px[:, 2]


def test_projection_and_membership_match_the_reference(tmp_path):
    z, meta = _golden()
    path = tmp_path / "0000.txt"
    path.write_text(C.calib_text(C.KITTI, "tracking"))
    calib = T.read_calib(str(path))
    for mine, ref in zip(calib, (z["P"], z["R0"], z["V2C"])):   # the reference's Calibration parsed the same text
        assert mine.dtype == np.float64 and np.array_equal(mine, ref)
    M = T.projection(calib)
    assert M.shape == (3, 4) and np.array_equal(M, R.projection(z["P"], z["R0"], z["V2C"]))
    np.testing.assert_allclose(M, z["P"] @ np.vstack([z["R0"] @ z["V2C"], [0, 0, 0, 1]]), rtol=0, atol=1e-9)
    pts, image = z["points"], tuple(float(v) for v in z["image"])
    assert pts.dtype == np.float32 and len(pts) == meta["points"] == 2000 and image == C.KITTI_IMAGE
    u, v = R.project(pts, M)
    front = pts[:, 0] > 2.0
    worst = max(np.abs(u - z["uv"][:, 0])[front].max(), np.abs(v - z["uv"][:, 1])[front].max())
    print("restatement against the reference's chain, %d points in front: %.3g px" % (front.sum(), worst))
    assert front.sum() > 1000 and (~front).sum() > 400 and worst <= 1e-9
    assert np.array_equal(R.inside(pts, M, image, C.EVERYWHERE), z["fov"]) and z["fov"].sum() == meta["in_image_and_front"] > 300
    assert len(z["rects"]) == meta["rects"] == 8 and (z["rects"][:, 2] > image[0]).any() and (z["rects"][:, 0] < 0).any()
    for i, rect in enumerate(z["rects"]):
        assert np.array_equal(R.inside(pts, M, image, rect), z["members"][i]) and z["members"][i].sum() == meta["members_per_rect"][i] > 0
        assert not R.undecided(pts, M, image, rect).any()


def test_restatement_agrees_with_the_three_product_chain_on_random_points():
    """200,000 random float32 points x 16 random rectangles under the KITTI-like calibration: u, v within 1e-9 px of the reference's chain
    for x > clip, the memberships equal, at most 1e-3 of the points undecided -- and on these inputs none."""
    g = np.random.RandomState(0)
    n = 200000
    x = g.uniform(-20, 80, n)
    pts = np.stack([x, -np.abs(x) * g.uniform(-1.2, 1.2, n), -np.abs(x) * g.uniform(-0.4, 0.4, n)], 1).astype(np.float32)
    M, (W, H) = T.projection(C.KITTI), C.KITTI_IMAGE
    u, v = R.project(pts, M)
    cu, cv = _chain(C.KITTI, pts)
    front = pts[:, 0] > 2.0
    worst = max(np.abs(u - cu)[front].max(), np.abs(v - cv)[front].max())
    n_und = n_dis = n_in = 0
    for _ in range(16):
        x0, y0 = g.uniform(-100, W - 100), g.uniform(-50, H - 80)
        rect = np.array([x0, y0, x0 + g.uniform(40, 500), y0 + g.uniform(30, 250)])
        with np.errstate(invalid="ignore"):
            ref = (cu < rect[2]) & (cu >= rect[0]) & (cv < rect[3]) & (cv >= rect[1]) & (cu < W) & (cu >= 0) & (cv < H) & (cv >= 0) & front
        mine, und = R.inside(pts, M, (W, H), rect), R.undecided(pts, M, (W, H), rect)
        n_in += int(mine.sum()); n_und += int(und.sum()); n_dis += int(((mine != ref) & ~und).sum())
    print("largest difference %.3g px, undecided %d, disagreements %d" % (worst, n_und, n_dis))
    assert worst <= 1e-9 and n_dis == 0 and n_in > 50000
    assert n_und <= 1e-3 * 16 * n and n_und == 0


def test_read_calib_accepts_both_styles(tmp_path):
    for style in ("tracking", "detection"):
        path = tmp_path / (style + ".txt")
        path.write_text(C.calib_text(C.OTHER, style))
        assert ("P2: " in path.read_text()) == (style == "detection")
        calib = T.read_calib(str(path))
        assert all(np.array_equal(a, b) for a, b in zip(calib, C.OTHER)) and calib.P.shape == (3, 4) and calib.R0.shape == (3, 3) and calib.V2C.shape == (3, 4)
    (tmp_path / "short.txt").write_text("P2: 1 2 3\nR0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 1 0 0 0 0 1 0 0 0 0 1 0\n")
    (tmp_path / "missing.txt").write_text("P2: 1 0 0 0 0 1 0 0 0 0 1 0\nR0_rect: 1 0 0 0 1 0 0 0 1\n")
    for bad in ("short.txt", "missing.txt"):
        with pytest.raises(ValueError):
            T.read_calib(str(tmp_path / bad))


def test_read_image_size_reads_the_png_header(tmp_path):
    head = C.png_header(1242, 375)
    assert len(head) == 33 and head[:8] == b"\x89PNG\r\n\x1a\n"
    (tmp_path / "a.png").write_bytes(head)
    assert T.read_image_size(str(tmp_path / "a.png")) == (1242, 375)
    (tmp_path / "b.png").write_bytes(head[:24])   # the 24 bytes it needs
    assert T.read_image_size(str(tmp_path / "b.png")) == (1242, 375)
    for name, data in (("c.png", head[:23]), ("d.png", b"\xff\xd8\xff\xe0" + head[4:]), ("e.png", head[:12] + b"IDAT" + head[16:])):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(ValueError):
            T.read_image_size(str(tmp_path / name))


def test_cli_parser_with_the_frustum_options():
    import make_kitti_dataset as M
    a = M.parse_args(["--kitti", "/k", "--out", "/o"])
    assert (a.from_bbox2d, a.calib_dir, a.image_dir, a.image_size, a.clip) == (False, "/k/training/calib", "/k/training/image_02", None, 2.0)
    a = M.parse_args(["--kitti", "/k", "--out", "/o", "--from-bbox2d", "--calib-dir", "/c", "--image-dir", "/i", "--image-size", "1242,375", "--clip", "1.5"])
    assert (a.from_bbox2d, a.calib_dir, a.image_dir, a.image_size, a.clip) == (True, "/c", "/i", (1242.0, 375.0), 1.5)
    for bad in (["--image-size", "1242"], ["--image-size", "0,375"], ["--image-size", "a,b"], ["--clip", "nan"]):
        with pytest.raises(SystemExit):
            M.parse_args(["--kitti", "/k", "--out", "/o"] + bad)


def test_header_declares_the_function_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "alignnet_hip.h")).read()
    assert re.search(r"#define\s+ALIGNNET_ABI_VERSION\s+1\b", text) and _capi.ABI_VERSION == 1
    m = re.search(r"\bint\s+alignnet_tracklet_extract_frustum\s*\(([^)]*)\)\s*;", text)
    assert m, "alignnet_tracklet_extract_frustum not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["alignnet_handle* h", "const int32_t* frames", "const double* rects", "const float* dz", "int32_t B", "const double* proj",
                    "const double* image", "double clip", "int64_t* offsets"]
    res, bound = _capi.SYMBOLS["alignnet_tracklet_extract_frustum"]
    P = ctypes.POINTER
    assert res is ctypes.c_int and bound[1:] == [P(ctypes.c_int32), P(ctypes.c_double), P(ctypes.c_float), ctypes.c_int32, P(ctypes.c_double),
                                                 P(ctypes.c_double), ctypes.c_double, P(ctypes.c_int64)]
    assert "alignnet_tracklet_extract_frustum" in _capi.LATE_SYMBOLS


def test_built_library_exports_the_frustum_symbol():
    lib = alignnet3d.load_library()
    assert hasattr(lib, "alignnet_tracklet_extract_frustum"), "not exported by " + alignnet3d.library_path()
    assert lib.alignnet_tracklet_extract_frustum.argtypes == _capi.SYMBOLS["alignnet_tracklet_extract_frustum"][1]
    assert callable(getattr(alignnet3d.Engine, "tracklet_extract_frustum"))


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_wrong_kernels_are_refused_by_the_gpu_tests_inputs():
    """The assertions of tests/test_frustum_gpu.py, evaluated on the CPU: the definition passes them, and each of the five wrong kernels of
    tests/frustum_ref.py fails the one made for it.  No GPU input has an undecided point (but the points placed exactly ON an edge)."""
    faces, near, clip, degen, edges = C.half_open_edges(), C.near_edges(), C.clip_and_behind(), C.degenerate_rects(), C.job_list_edges(PER_PASS)
    # the definition
    assert _equal(C.members(faces), faces["expected"]) and faces["expected"][0].sum() == 2 * 3 and faces["expected"][1].sum() == 12 + 2 * 3 + 1
    assert _equal(C.members(clip), [clip["expected"]] * 2) and clip["expected"].sum() == 70
    assert len(near["chosen"]) == 16 and near["kept"].sum() == 8 and len(near["scans"]) == 9
    for job, (m, c, keep) in enumerate(zip(C.members(near), near["chosen"], near["kept"])):
        assert m[c] == keep, job
    W, H = C.KITTI_IMAGE
    u, v = R.project(degen["scans"][0], degen["proj"])
    m = C.members(degen)
    in_rect = (u >= W) & (u < degen["rects"][0, 0, 2]) & (v >= 200) & (v < H) & (degen["scans"][0][:, 0] > 2)
    assert m[0].sum() > 10 and in_rect.sum() > 10 and not (m[0] & in_rect).any() and (u[m[0]] < W).all() and (v[m[0]] < H).all()
    assert [int(x.sum()) for x in m[1:]] == [0, 0, 0] and ((u >= W + 10) & (u < W + 300) & (v >= 50) & (v < 300)).sum() > 10
    counts = np.array([int(x.sum()) for x in C.members(edges)]).reshape(-1, 2)
    assert (counts[:-1] > 0).mean() > 0.8 and not counts[-1].any()
    assert (edges["frames"] == 0).sum() == 2 * PER_PASS + 1 and (edges["frames"] == 1).sum() == PER_PASS + 1 and not (edges["frames"] == 2).any()
    # the wrong kernels
    wrong_near = C.members(near, R.inside_f32)
    assert all(w[c] != m[c] for w, m, c in zip(wrong_near, C.members(near), near["chosen"]))          # an all-float32 projection: every job
    assert not _equal(C.members(faces, R.inside_closed), faces["expected"])                              # closed upper edges
    assert int((C.members(faces, R.inside_closed)[0] != faces["expected"][0]).sum()) == 2                # ... the points ON xmax and ON ymax
    assert int((C.members(faces, R.inside_closed)[1] != faces["expected"][1]).sum()) == 2                # ... the points ON u = W and ON v = H
    assert int((C.members(clip, R.inside_noclip)[0] != clip["expected"]).sum()) == 60 + 60               # no clip test: the mirrored and the near points
    assert int((C.members(faces, R.inside_noclip)[1] != faces["expected"][1]).sum()) == 2                # ... and x == clip, one step below
    assert (C.members(degen, R.inside_noimage)[0] & in_rect).sum() == in_rect.sum() and C.members(degen, R.inside_noimage)[1].sum() > 10   # no image test
    wrong_edges = C.members(edges, frame0_calibration=True)
    on_1 = np.flatnonzero(np.ravel(edges["frames"]) == 1)
    assert sum(not np.array_equal(wrong_edges[j], C.members(edges)[j]) for j in on_1) > 0.8 * len(on_1)  # frame 0's calibration for every frame
    # undecided points: none, but those placed exactly on an edge (gap == 0, decided by exact arithmetic)
    for case in (C.random_frames(CHUNK, 4), C.random_frames(CHUNK, 3), near, degen, edges):
        n, und = C.undecided_count(case)
        assert n > 0 and und == 0
    for case in (faces, clip):
        assert C.undecided_count(case, exact=True)[1] == 0
    assert C.undecided_count(faces)[1] > 0
    easy = C.random_frames(CHUNK, 4)
    assert sum(int(x.sum()) for x in C.members(easy)) > 300 and _equal(C.members(easy, R.inside_f32), C.members(easy)) and _equal(C.members(easy, R.inside_closed), C.members(easy))
