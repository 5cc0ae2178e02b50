"""CPU: the binned cast of the scene generator (alignnet_set_option "scene_cast", csrc/alignnet_scene.hip) wherever no GPU is needed: the header,
the ctypes table, the command line and scenes.generate's `cast`, the compiler's resource remarks of the new kernels and of the scan kernel they must
leave alone, and the helper the GPU tests take their tile-list bounds from (tests/scene_bin_ref.py)."""
import os
import re
import sys

import numpy as np
import pytest

from alignnet3d import _capi
from alignnet3d import scenes as S
from tests import scene_bin_ref as BR
from tests import scene_cases as C
from tests import scene_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")

# the two scene_cast_kernel instantiations as the commit before the binned cast built them (hipcc -O3, gfx950): VGPRs, scratch bytes per lane,
# static LDS bytes (the 44 KiB stage is dynamic LDS on top, sized by the host for both casts alike)
SCAN_KERNEL_BEFORE = dict(vgprs=80, scratch=0, lds=16)
NEW_KERNELS = ("scene_bin_tally_kernel", "scene_bin_offsets_kernel", "scene_bin_fill_kernel", "scene_bincast_kernel")


def test_header_declares_and_capi_binds_the_binned_read_back():
    text = open(os.path.join(ROOT, "include", "alignnet_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint alignnet_debug_scene_cast_binned\s*\(([^)]*)\)", code)
    assert m, "alignnet_debug_scene_cast_binned not declared"
    assert len(m.group(1).split(",")) == 11 == len(_capi.SYMBOLS["alignnet_debug_scene_cast_binned"][1])
    m0 = re.search(r"\bint alignnet_debug_scene_cast\s*\(([^)]*)\)", code)
    assert m0 and len(m0.group(1).split(",")) == 9 == len(_capi.SYMBOLS["alignnet_debug_scene_cast"][1])      # the scan's read-back keeps its signature
    for key in ('"scene_cast"', '"scene_binned_clouds"', '"icp_search"'):
        assert key in text, key
    assert "#define ALIGNNET_ABI_VERSION 1\n" in text and _capi.ABI_VERSION == 1
    import alignnet3d
    assert hasattr(alignnet3d.load_library(), "alignnet_debug_scene_cast_binned")
    assert "scene_bin" in alignnet3d.Engine.PROFILED_KERNELS
    names = re.search(r"kProfKernelNames\[PK_COUNT\]\s*=\s*\{(.*?)\}", open(os.path.join(PKG, "csrc", "engine.h")).read(), re.S).group(1)
    assert tuple(re.findall(r'"(\w+)"', names)) == tuple(alignnet3d.Engine.PROFILED_KERNELS)


def test_command_line_and_generate_take_the_cast_by_name():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import make_synth_dataset as M
    ap = M.build_parser()
    assert ap.parse_args(["--out", "x"]).cast == "scan"
    for name in ("scan", "binned", "auto"):
        assert ap.parse_args(["--out", "x", "--cast", name]).cast == name
    with pytest.raises(SystemExit):
        ap.parse_args(["--out", "x", "--cast", "fast"])
    assert S.CASTS == {"scan": 0, "binned": 1, "auto": 2}

    class Untouchable:
        def __getattribute__(self, name):
            raise AssertionError("engine touched (%s) before the cast name was checked" % name)

    with pytest.raises(ValueError, match="cast"):
        S.generate(Untouchable(), [S.draw_scene(3, "cars")], cast="fast")


def _remarks():
    path = os.path.join(PKG, "csrc", "alignnet_scene.remarks")
    assert os.path.exists(path), "no resource remarks next to the objects: csrc/Makefile writes them"
    rows = re.findall(r"Function Name: (\S+).*?[^A]VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+).*?"
                      r"LDS Size \[bytes/block\]: (\d+)", open(path).read(), re.S)
    return {name: dict(vgprs=int(v), scratch=int(sc), sgpr_spill=int(ss), vgpr_spill=int(vs), lds=int(l)) for name, v, sc, ss, vs, l in rows}


def test_new_kernels_use_no_scratch_and_the_scan_kernel_is_unchanged():
    rem = _remarks()
    for key in NEW_KERNELS:
        found = {n: r for n, r in rem.items() if key in n}
        assert len(found) == (2 if key == "scene_bincast_kernel" else 1), (key, sorted(rem))
        for n, r in found.items():
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (n, r)
    scan = {n: r for n, r in rem.items() if "scene_cast_kernel" in n}
    assert len(scan) == 2
    for n, r in scan.items():
        assert {k: r[k] for k in SCAN_KERNEL_BEFORE} == SCAN_KERNEL_BEFORE and r["vgpr_spill"] == 0, (n, r)
    # three workgroups per CU as for the scan: no more static LDS than it (both get the same dynamic stage), no more registers
    for n, r in rem.items():
        if "scene_bincast_kernel" in n:
            assert r["lds"] <= SCAN_KERNEL_BEFORE["lds"] and r["vgprs"] <= SCAN_KERNEL_BEFORE["vgprs"], (n, r)
    src = open(os.path.join(PKG, "csrc", "alignnet_scene.hip")).read()
    assert src.count("const size_t lds = (size_t)L * sizeof(SceneTri);") == 1      # one stage size for every cast launch


@pytest.mark.parametrize("name", sorted(C.CASES) + sorted(BR.EXTRA))
def test_tile_bounds_are_consistent(name):
    """What a tile's rays hit (the restatement's record) never exceeds what the dilated intervals allow its list to hold."""
    lower, upper = BR.case_bounds(name)
    first, count = BR.reference(name)["window"]
    assert len(lower) == len(upper) == BR.tiles_of(count)
    assert np.all(lower <= upper), (name, np.flatnonzero(lower > upper)[:10])
    if name == "over_sensor":
        assert len(upper) == BR.FULL_TILES == 563
    if name == "empty":
        assert len(upper) == 0


def test_two_blobs_has_empty_tiles_inside_its_window():
    ref = BR.reference("two_blobs")
    lower, upper = BR.case_bounds("two_blobs")
    assert ref["window"] == (2779, 372) and len(upper) == 47
    assert len(ref["rays"]) == 1380 and len(ref["undecided"]) == 0
    assert (upper == 0).sum() >= 20
    # ... strictly inside: the first and the last tile hold triangles
    assert upper[0] > 0 and upper[-1] > 0 and lower.sum() > 0


def test_interval_helper_restates_the_window():
    """The per-triangle intervals give back scene_ref.window's windows: the union of the columns they cover is the window's column set."""
    for name in ("car_6m", "wrap_plus180", "zero_area", "two_blobs"):
        v, f, scale, pose = BR.case(name)
        ref = BR.reference(name)
        kind, ca, cb = BR.triangle_intervals(ref["posed"], f, 1e-6)
        assert not (kind == 2).any()
        cov = np.zeros(R.HRES, bool)
        for i in np.flatnonzero(kind == 1):
            cov[np.arange(ca[i], cb[i] + 1) % R.HRES] = True
        cols = R.window_columns(*ref["window"])
        assert cov[cols[0]] and cov[cols[-1]] and not cov[np.setdiff1d(np.arange(R.HRES), cols)].any(), name
    # the two faces with a repeated vertex have N = 0 exactly and reach nothing (the collinear one need not: its posed normal may round off zero)
    assert (BR.triangle_intervals(BR.reference("zero_area")["posed"], BR.case("zero_area")[1], 1e-6)[0][:2] == 0).all()
    v, f = BR.car2064()
    assert len(f) == 2064
