"""Inputs of tests/test_scene_rows_cpu.py and tests/test_scene_rows_gpu.py that tests/scene_cases.py does not hold: a handful of triangles each,
placed where the band mask of the cast by elevation band (tests/scene_rows_ref.py) can go wrong.  A case is (vertices, faces, scale, pose) as in
scene_cases; vertices are in metres (scale 1, pose 0).  sensor() is the custom table set of case (e)."""
import functools

import numpy as np

from alignnet3d import scenes as S
from tests import scene_cases as C
from tests import scene_ref as R

_DX, _DY, _DZ = S.sensor_tables()
_ID = (0.0, 0.0, 0.0, 0.0)


def _faces(n):
    return np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def _thin_near_axis():
    """(a) A 20 m long, 5 cm wide strip 30 cm below the sensor's height that passes the z axis at 2 m: its vertices are 10 m away (slope -0.03,
    -1.7 degrees) but the middle of its long edges is at rho = 2 m (slope -0.15, -8.5 degrees), so rays hit it six rows below the rows of its vertices.
    A second, ordinary triangle stands behind it."""
    strip = [[-10.0, 2.0, -0.3], [10.0, 2.0, -0.3], [10.0, 2.05, -0.3], [-10.0, 2.0, -0.3], [10.0, 2.05, -0.3], [-10.0, 2.05, -0.3]]
    back = [[-1.0, 9.0, -1.0], [1.0, 9.0, -1.0], [0.0, 9.0, 1.5]]
    return np.array(strip + back), _faces(3), 1.0, _ID


def _straddles_zero():
    """(b) z from -1 to +1 at 8 m: the slope changes sign inside the triangle; one triangle wholly below and one wholly above next to it."""
    v = [[-1.0, 8.0, -1.0], [1.0, 8.5, -0.2], [0.2, 7.5, 1.0],
         [2.0, 8.0, -1.5], [3.0, 8.0, -1.4], [2.5, 8.5, -0.1],
         [-3.0, 8.0, 0.1], [-2.0, 8.0, 1.4], [-2.5, 8.5, 1.5]]
    return np.array(v), _faces(3), 1.0, _ID


def _over_and_under():
    """(c) Two large horizontal triangles whose xy projection holds the z axis, 3 m above and 2 m below the sensor: every column, every band."""
    v = [[-40.0, -30.0, 3.0], [40.0, -30.0, 3.0], [0.0, 50.0, 3.0],
         [-35.0, -25.0, -2.0], [0.0, 45.0, -2.0], [35.0, -25.0, -2.0]]
    return np.array(v), _faces(2), 1.0, _ID


def _exact_boundary():
    """(d) Column 2250 looks along +y with dir = (0, 120) exactly.  Face 0 hangs from a horizontal edge at y = 7.5 = 120 / 16, z = dir_z[40] / 16,
    whose nearest point to the axis is its middle: the edge's largest slope is exactly row 40's, the first row of band 5, which no other point of
    the face reaches (dir_z[40] / 120 * 120 gives dir_z[40] back in fp64, so the rule holds there with no margin at all).  Face 1
    has its top vertex exactly on the ray (row 24, column 2300) -- the first row of band 3 -- at 1 / 16 of the direction, everything else of it
    below."""
    z0 = _DZ[40] / 16.0
    f0 = [[-0.4, 7.5, z0], [0.4, 7.5, z0], [0.0, 7.5, z0 - 0.5]]
    top = np.array([_DX[2300], _DY[2300], _DZ[24]]) / 16.0
    side = np.array([_DY[2300], -_DX[2300], 0.0]) / 120.0
    f1 = [top, top + 0.3 * side - [0, 0, 0.6], top - 0.3 * side - [0, 0, 0.6]]
    return np.array(f0 + f1), _faces(2), 1.0, _ID


@functools.lru_cache(None)
def sensor():
    """(e) dir_z a permutation of the default (non-monotone), dir_x / dir_y the default directions with a norm that varies by column, 84 .. 156."""
    perm = np.random.RandomState(5).permutation(R.VRES)
    scale = 1.0 + 0.3 * np.sin(0.37 * np.arange(R.HRES))
    return _DX * scale, _DY * scale, _DZ[perm].copy()


CASES = {
    "thin_near_axis": _thin_near_axis(),
    "straddles_zero": _straddles_zero(),
    "over_and_under": _over_and_under(),
    "exact_boundary": _exact_boundary(),
    "custom_sensor": (*C.ellipsoid(1), 1.0, C.polar(9.0, 31.0)),
}
NAMES = tuple(CASES)
OLD_NAMES = C.CAST_CASES + C.EDGE_CASES + C.WRAP_CASES


def case(name):
    return CASES[name] if name in CASES else C.CASES[name]


def tables(name):
    return sensor() if name == "custom_sensor" else S.sensor_tables()


@functools.lru_cache(None)
def reference(name):
    """The restatement's cloud of a case on its own window, with the case's sensor tables (scene_cases.reference for its names)."""
    if name in C.CASES:
        return C.reference(name)
    v, f, scale, pose = CASES[name]
    return R.cloud(v, f, scale, pose, tables=tables(name))
