"""GPU: the argument checks of the ICP entry points (csrc/alignnet_icp.hip), through the C API as tests/test_icp_plane_gpu.py's flags test calls it.
Every rejected call returns non-zero and leaves in alignnet_last_error the text stated here, the entry point's name at its head where the check is
the entry's own ("icp:" / "icp_plane:" where it is the shared driver's).  All of them return before any launch.  Then, on the handle that saw every
one of these errors, one valid call of icp_refine, icp_refine_rows and icp_plane_refine returns the bytes a fresh engine returns.
Inputs: two pairs of 3 and 4 points, and a dataset of the same two pairs for the rows forms."""
import ctypes as C

import numpy as np
import pytest

import alignnet3d
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu

HOST = ("p1", "p2", "off", "B", "init", "radius")
ROWS = ("rows", "B", "init", "radius")
OUT = ("out", "fit", "rmse", "it")
PAIR = ("p1", "n1", "p2", "n2", "init", "radius")
ENTRIES = {   # the arguments behind the handle, in the order of include/alignnet_hip.h
    "alignnet_icp_refine": HOST + ("its",) + OUT,
    "alignnet_icp_register": HOST + ("its", "flags") + OUT,
    "alignnet_icp_plane_register": HOST + ("normal_radius", "its", "flags") + OUT,
    "alignnet_icp_refine_dataset": ROWS + ("its",) + OUT,
    "alignnet_icp_register_dataset": ROWS + ("its", "flags") + OUT,
    "alignnet_icp_plane_register_dataset": ROWS + ("normal_radius", "its", "flags") + OUT,
    "alignnet_debug_icp_scan": PAIR + ("flags", "lds_points", "index", "dist2", "inlier", "paths", "used", "fit", "rmse"),
    "alignnet_debug_icp_grid": PAIR + ("flags", "index", "dist2", "inlier", "paths", "edge", "occ", "big", "fit", "rmse"),
    "alignnet_debug_icp_plane": PAIR + ("normal_radius", "flags", "normals", "neighbours", "index", "dist2", "inlier", "residual", "sums", "update", "fit", "rmse"),
}
POINTERS = {np.dtype(np.float32): C.c_float, np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32, np.dtype(np.int64): C.c_int64}
NULL_BOUNDS, DECREASING, NULL_BLOB = "{fn}: null offsets or B < 1", "{fn}: offsets must be non-decreasing", "{fn}: null point blob"
NULL_IO, FLAGS = "{run}: null init / out", "{fn}: unknown flags 2 (bit 0 = full rotation is the only one)"
BOUNDS = {"icp": "icp: radius must be > 0 and its >= 0", "icp_plane": "icp_plane: radius and normal_radius must be > 0 and its >= 0"}


def _inputs():
    rng = np.random.default_rng(11)
    srcs = [rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32) for n in (3, 4)]
    c, s = np.cos(0.02), np.sin(0.02)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    dsts = [(p.astype(np.float64) @ Rz.T + [0.01, -0.005, 0.002]).astype(np.float32) for p in srcs]
    return srcs, dsts, [np.eye(4), np.eye(4)]


def _values(srcs, dsts, inits):
    """Every argument's valid value: arrays (passed as pointers) and scalars.  n1 / n2 / the debug outputs are pair 0's."""
    off = np.array([[0, 0], [3, 3], [7, 7]], np.int64)
    z = lambda n, t: np.zeros(n, t)
    return dict(p1=np.ascontiguousarray(np.concatenate(srcs)), p2=np.ascontiguousarray(np.concatenate(dsts)), off=off, B=2, rows=np.array([1, 0], np.int32),
                init=np.ascontiguousarray(np.stack(inits).reshape(2, 16)), radius=0.1, normal_radius=0.3, its=30, flags=0, lds_points=0, n1=3, n2=3,
                out=z(32, np.float64), fit=z(2, np.float64), rmse=z(2, np.float64), it=z(2, np.int32),
                index=z(3, np.int32), dist2=z(3, np.float64), inlier=z(3, np.int32), paths=z(3, np.int32), used=z(1, np.int32), edge=z(1, np.float64),
                occ=z(1, np.int32), big=z(1, np.int32), normals=z(9, np.float64), neighbours=z(3, np.int32), residual=z(3, np.float64),
                sums=z(29, np.float64), update=z(16, np.float64))


def _rejected(eng, fn, values, label, message, **change):
    v = dict(values, **change)
    args = [v[k].ctypes.data_as(C.POINTER(POINTERS[v[k].dtype])) if isinstance(v[k], np.ndarray) else v[k] for k in ENTRIES[fn]]
    rc = getattr(eng._lib, fn)(eng._h, *args)
    got = eng._lib.alignnet_last_error(eng._h).decode()
    run = "icp_plane" if "plane" in fn else "icp"
    want = message.format(fn=fn, run=run)
    assert rc != 0 and got == want, (fn, label, rc, got, want)


def _valid_calls(eng, srcs, dsts, inits):
    res = []
    for constrained in (True, False):
        res.append(eng.icp_refine(srcs, dsts, inits, constrained=constrained))
        res.append(eng.icp_refine_rows([1, 0], [inits[1], inits[0]], constrained=constrained))
        res.append(eng.icp_plane_refine(srcs, dsts, inits, constrained=constrained))
    return [r[k].tobytes() for r in res for k in ("transforms", "fitness", "rmse", "iterations")]


def _upload(eng, srcs, dsts):
    off = np.array([[0, 0], [3, 3], [7, 7]], np.int64)
    eng.upload_dataset(np.concatenate(srcs), np.concatenate(dsts), off, np.zeros((2, 12), np.float32))


def test_rejected_arguments_keep_their_messages_and_the_handle(gpu_required):
    srcs, dsts, inits = _inputs()
    eng = alignnet3d.Engine(small_cfg(N=64, nb=12))
    v = _values(srcs, dsts, inits)
    # the rows forms before any upload
    for fn in ENTRIES:
        if fn.endswith("_dataset"):
            _rejected(eng, fn, v, "no dataset", "{fn}: no dataset uploaded")
    _upload(eng, srcs, dsts)
    for fn, names in ENTRIES.items():
        plane, bounds = "plane" in fn, BOUNDS["icp_plane" if "plane" in fn else "icp"]
        if "flags" in names:
            _rejected(eng, fn, v, "flags 2", FLAGS, flags=2)
        if "off" in names:      # clouds from the host
            _rejected(eng, fn, v, "decreasing source offsets", DECREASING, off=np.array([[0, 0], [3, 3], [2, 7]], np.int64))
            _rejected(eng, fn, v, "decreasing target offsets", DECREASING, off=np.array([[0, 0], [3, 3], [7, 2]], np.int64))
            _rejected(eng, fn, v, "B 0", NULL_BOUNDS, B=0)
            _rejected(eng, fn, v, "null offsets", NULL_BOUNDS, off=None)
        if "rows" in names:     # clouds of the dataset
            _rejected(eng, fn, v, "null rows", "{fn}: null rows or B < 1", rows=None)
            _rejected(eng, fn, v, "B 0", "{fn}: null rows or B < 1", B=0)
            _rejected(eng, fn, v, "row -1", "{fn}: row -1 out of range", rows=np.array([1, -1], np.int32))
            _rejected(eng, fn, v, "row n", "{fn}: row 2 out of range", rows=np.array([2, 0], np.int32))
        if "n1" in names:       # the read-backs of one pair
            _rejected(eng, fn, v, "n1 -1", "{fn}: n1 / n2 out of range", n1=-1)
            _rejected(eng, fn, v, "null index", "{fn}: null output", index=None)
            _rejected(eng, fn, v, "null inlier", "{fn}: null output", inlier=None)
        if "lds_points" in names:
            _rejected(eng, fn, v, "lds_points", "{fn}: lds_points must be in [0, 4266] (0 = as shipped)", lds_points=4267)
        if "p1" in names:
            _rejected(eng, fn, v, "null source blob", NULL_BLOB, p1=None)
            _rejected(eng, fn, v, "null target blob", NULL_BLOB, p2=None)
        _rejected(eng, fn, v, "null init", NULL_IO, init=None)
        if "out" in names:
            _rejected(eng, fn, v, "null out", NULL_IO, out=None)
        _rejected(eng, fn, v, "radius 0", bounds, radius=0.0)
        if "its" in names:
            _rejected(eng, fn, v, "its -1", bounds, its=-1)
        if plane:
            _rejected(eng, fn, v, "normal_radius 0", bounds, normal_radius=0.0)
    # the handle is left usable: the bytes of a fresh engine
    after = _valid_calls(eng, srcs, dsts, inits)
    eng.close()
    fresh = alignnet3d.Engine(small_cfg(N=64, nb=12))
    _upload(fresh, srcs, dsts)
    assert after == _valid_calls(fresh, srcs, dsts, inits)
    fresh.close()
