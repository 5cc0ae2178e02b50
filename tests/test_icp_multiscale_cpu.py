"""CPU: multi-scale ICP as restated in tests/icp_multiscale_ref.py (the definition of alignnet_icp_multiscale_register*): the declaration, export and
binding of the new entry points, the drop-in's option, the restatement's own properties, the conditions the inputs of tests/test_icp_multiscale_gpu.py
meet, and that two plausible wrong pyramids move the level clouds by more than that test's bars.  No compute calls (there is no GPU and no CPU
fallback)."""
import functools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import global_reg_ref as G
from tests import icp_multiscale_ref as M
from tests import icp_plane_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
NAMES = (("alignnet_icp_multiscale_register", 18), ("alignnet_icp_multiscale_register_dataset", 16), ("alignnet_debug_voxel_pyramid", 10))


@functools.lru_cache(maxsize=None)
def _car():
    return M.car_scan()


@functools.lru_cache(maxsize=None)
def _far_cloud():
    return M.far_cloud()


@functools.lru_cache(maxsize=None)
def _small(k):
    seed, dist = M.SMALL_PAIRS[k]
    return P.car_pair(dist, seed)


# ---- 1. the surface ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    from alignnet3d import _capi
    import alignnet3d
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alignnet_hip.h")).read(), flags=re.S)
    for name, nargs in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, name + " not declared in include/alignnet_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_capi.SYMBOLS[name][1]), name
    lib = alignnet3d.load_library()
    for name, _ in NAMES:
        assert hasattr(lib, name)
    exported = subprocess.run(["nm", "-D", "--defined-only", alignnet3d.library_path()], capture_output=True, text=True, check=True).stdout
    for name, _ in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M), name + " is not exported by the library"
    for method in ("icp_multiscale_refine", "icp_multiscale_refine_rows", "debug_voxel_pyramid"):
        assert callable(getattr(alignnet3d.Engine, method))
    assert "icp_pyramid" in alignnet3d.Engine.PROFILED_KERNELS
    assert "alignnet_multiscale.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def test_pyramid_kernels_use_no_scratch():
    """The resource remarks the build leaves next to the object: three kernels, none with scratch or spills."""
    text = open(os.path.join(PKG, "csrc", "alignnet_multiscale.remarks")).read()
    assert len(re.findall(r"Function Name: \S*ms_(?:sort|scan|emit)_kernel", text)) == 3
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)] == [0, 0, 0]
    assert [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", text)] == [0, 0, 0]


def test_icp_multiscale_option():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import train

    def conf(**ev):
        return types.SimpleNamespace(evaluation=types.SimpleNamespace(**ev))

    def ms(**kw):
        return conf(icp_multiscale=types.SimpleNamespace(**kw))

    assert train.icp_multiscale_option(conf()) is None
    assert train.icp_multiscale_option(conf(icp_multiscale=False)) is None
    assert train.icp_multiscale_option(types.SimpleNamespace()) is None
    good = train.icp_multiscale_option(ms(voxel_sizes=[0.2, 0.1, 0], radii=[0.4, 0.2, 0.1], its=[30, 30, 30]))
    assert good == ([0.2, 0.1, 0.0], [0.4, 0.2, 0.1], [30, 30, 30])
    assert train.icp_multiscale_option(conf(icp_multiscale=dict(voxel_sizes=[-1], radii=[0.1], its=[0]))) == ([-1.0], [0.1], [0])
    assert len(train.icp_multiscale_option(ms(voxel_sizes=[0.1] * 8, radii=[0.1] * 8, its=[1] * 8))[0]) == 8
    bad = (dict(voxel_sizes=[0.2, 0.1], radii=[0.4], its=[30, 30]),             # unequal lengths
           dict(voxel_sizes=[], radii=[], its=[]),                                # empty
           dict(voxel_sizes=[0.1] * 9, radii=[0.1] * 9, its=[1] * 9),             # L > 8
           dict(voxel_sizes=[0.2], radii=[0.0], its=[30]),                        # a radius <= 0
           dict(voxel_sizes=[0.2], radii=[-0.1], its=[30]),
           dict(voxel_sizes=[0.2], radii=[0.1], its=[-1]),                        # a negative budget
           dict(voxel_sizes=[0.2], radii=[0.1]),                                  # a list missing
           dict(voxel_sizes=0.2, radii=[0.1], its=[30]),                          # not a list
           dict(voxel_sizes=[0.2], radii=[0.1], its=[1.5]),                       # a fractional budget
           dict(voxel_sizes=[float("nan")], radii=[0.1], its=[1]))
    for kw in bad:
        with pytest.raises(ValueError, match=r"evaluation\.icp_multiscale"):
            train.icp_multiscale_option(ms(**kw))


# ---- 2. the restatement's own properties -------------------------------------------------------------------------------------------------------
def test_level_without_voxel_is_the_raw_cloud():
    src = _small(0)[0]
    for v in (0.0, -1.0):
        assert M.level_cloud(src, v) is not None and np.array_equal(M.level_cloud(src, v), src)
        lv = M.pyramid(src, [v])[0]
        assert lv["voxels"] is None and np.array_equal(lv["points"], src) and np.all(lv["counts"] == 1)


@pytest.mark.parametrize("estimate", ("point", "plane", "generalized"))
@pytest.mark.parametrize("constrained", (True, False))
def test_one_raw_level_is_the_single_scale_restatement(estimate, constrained):
    src, dst, truth = _small(0)
    init = M.disturbed_init(src, truth, 1)
    r = M.icp_multiscale(src, dst, init, [0.0], [0.1], [6], estimate, 0.3, constrained)
    T, fit, rmse, k = M.icp_single(src, dst, init, 0.1, 6, estimate, 0.3, constrained)
    assert np.array_equal(r["transform"], T) and r["fitness"] == fit and r["rmse"] == rmse and r["iterations"].tolist() == [k]
    assert r["level_sizes"].tolist() == [[len(src), len(dst)]]


def test_voxels_partition_the_input_and_sizes_fall_with_the_edge():
    for pc, voxels in ((_car()[0], M.CAR_VOXELS), (_car()[1], M.CAR_VOXELS), (_far_cloud(), M.FAR_VOXELS), (M.lattice(), (0.5, 0.25, 0.125))):
        sizes = []
        for v in voxels:
            d = G.voxel_downsample(pc, v)
            assert d["counts"].sum() == len(pc) and d["counts"].min() >= 1
            key = (d["voxels"][:, 0] << 42) | (d["voxels"][:, 1] << 21) | d["voxels"][:, 2]
            assert np.all(np.diff(key) > 0)                      # every voxel once, ascending (ix, iy, iz)
            # every point lies in the voxel it was counted in: the sums of all voxels are the sum of all points
            np.testing.assert_allclose((d["points"] * d["counts"][:, None]).sum(0), pc.astype(np.float64).sum(0), rtol=1e-9)
            sizes.append(len(d["points"]))
        assert sizes == sorted(sizes), sizes                      # (the voxel lists run from coarse to fine)


def test_schedule_errors():
    src, dst, truth = _small(0)
    for vs, rd, it in (([], [], []), ([0.1] * 9, [0.1] * 9, [1] * 9), ([0.1], [0.0], [1]), ([0.1], [0.1], [-1]), ([0.1, 0.2], [0.1], [1, 1])):
        with pytest.raises(ValueError):
            M.icp_multiscale(src, dst, truth, vs, rd, it)


def test_empty_level_keeps_the_transform():
    src, dst, truth = _small(0)
    for s, d in ((src[:0], dst), (src, dst[:0])):
        for estimate in ("point", "plane", "generalized"):
            r = M.icp_multiscale(s, d, truth, [0.2, 0.0], [0.2, 0.1], [5, 5], estimate)
            assert np.array_equal(r["transform"], truth) and r["iterations"].tolist() == [0, 0] and r["fitness"] == 0.0 and r["rmse"] == 0.0


# ---- 3. conditions the GPU test's inputs meet ---------------------------------------------------------------------------------------------------
def test_committed_inputs_are_decided():
    """At most FACE_REF_CAP of a cloud's points within FACE bin widths of a voxel face, for every (cloud, voxel size) the GPU test compares."""
    cases = [("car source", _car()[0], M.CAR_VOXELS), ("car target", _car()[1], M.CAR_VOXELS), ("far cloud", _far_cloud(), M.FAR_VOXELS)]
    fs, fd, _ = M.far_pair()
    cases += [("far pair source", fs, M.FAR_VOXELS), ("far pair target", fd, M.FAR_VOXELS)]
    for k in range(len(M.SMALL_PAIRS)):
        cases += [("small %d source" % k, _small(k)[0], M.CAR_VOXELS), ("small %d target" % k, _small(k)[1], M.CAR_VOXELS)]
    for name, pc, voxels in cases:
        for v in voxels:
            share = M.undecided_share(pc, v)
            print("%s at %g: %d points, undecided share %.2e" % (name, v, len(pc), share))
            assert share <= M.FACE_REF_CAP, (name, v, share)


def test_why_the_far_voxel_sizes_are_not_round():
    """At FAR a round voxel size puts points exactly on faces whatever the seed (tests/icp_multiscale_ref.py: FAR_VOXELS)."""
    assert M.undecided_share(_far_cloud(), 0.05) > M.FACE_CAP


def test_lattice_is_exact_and_on_faces():
    """Multiples of 2^-4 at voxel 2^-3: every quotient is a multiple of 1/2 held exactly, 7 / 8 of the points lie exactly on a face."""
    pc = M.lattice()
    v = 0.125
    q = pc.astype(np.float64) * 16
    assert np.array_equal(q, np.round(q)) and pc.min() == 0.0
    pre = (pc.astype(np.float64) - (pc.min(0).astype(np.float64) - v / 2)) / v
    assert np.array_equal(pre * 2, np.round(pre * 2))            # exact: nothing was rounded
    assert np.array_equal(pre, q / 2 + 0.5)
    share = M.on_face_share(pc, v)
    print("lattice: %.1f %% of the points on a voxel face" % (100 * share))
    assert 0.86 < share < 0.89
    d = G.voxel_downsample(pc, v)
    assert np.array_equal(d["voxels"], np.unique(np.floor(q / 2 + 0.5).astype(np.int64), axis=0))   # the closed lower face: a point ON a face belongs above


# ---- 4. teeth ----------------------------------------------------------------------------------------------------------------------------------
def test_wrong_pyramids_exceed_the_gpu_bars():
    """The GPU test's bars: voxels and counts equal, fp64 means within MEAN_TOL relative, the float32 cloud equal to float32(device mean).  A mean summed
    in float32 misses the second by five orders and the third at most points; an origin at the minimum changes the voxels themselves."""
    src = _car()[0]
    for v in M.CAR_VOXELS:
        ref = M.pyramid(src, [v])[0]
        wrong = M.level_cloud_fp32_sum(src, v)
        multi = ref["counts"] > 2          # (one or two float32 terms add exactly or round once, as the fp64 sum's rounding to float32 does)
        moved = np.any(wrong != ref["points"], 1)
        rel = np.abs(wrong.astype(np.float64) - ref["means"]).max() / np.abs(ref["means"]).max()
        print("voxel %g: float32 sum moves %d of %d level points (%d hold more than two), by %.1e relative" % (v, moved.sum(), len(moved), multi.sum(), rel))
        assert rel > 1e4 * M.MEAN_TOL and moved.sum() >= 0.1 * multi.sum() > 0
        shifted = M.level_cloud_origin_at_min(src, v)
        same = len(shifted) == len(ref["points"]) and np.array_equal(shifted, ref["points"])
        print("voxel %g: origin at the minimum gives %d level points instead of %d" % (v, len(shifted), len(ref["points"])))
        assert not same
        if len(shifted) == len(ref["points"]):
            assert np.abs(shifted - ref["points"]).max() > 1e-3
