"""Inputs shared by tests/test_scene_cpu.py and tests/test_scene_gpu.py: small meshes, poses, and the restatement's results on them
(tests/scene_ref.py), computed once per process.  A case is (vertices, faces, scale, pose); vertices are handed to the engine as they
are (the C ABI does not normalise), so an ellipsoid in metres goes in with scale 1."""
import functools

import numpy as np

from alignnet3d import scenes as S
from tests import scene_ref as R


@functools.lru_cache(None)
def icosphere(level):
    """Unit icosphere: 20 * 4^level triangles."""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int32)


def ellipsoid(level):
    """Half-axes 3 x 1.2 x 1.0 m."""
    v, f = icosphere(level)
    return v * np.array([3.0, 1.2, 1.0]), f


def polar(dist, bearing_deg, yaw=0.3, z=0.0):
    """Pose at `dist` metres on the bearing h (the sensor's azimuth: x = sin h, y = cos h)."""
    h = np.deg2rad(bearing_deg)
    return (dist * np.sin(h), dist * np.cos(h), z, yaw)


@functools.lru_cache(None)
def car():
    v, f, _ = S.load_mesh("builtin", "car", 1)
    return v, f


@functools.lru_cache(None)
def person():
    v, f, _ = S.load_mesh("builtin", "person", 1)
    return v, f


def _edge_cases():
    ev, ef = ellipsoid(1)
    out = {}
    for n in (1, 63, 64, 65):
        out["first%d" % n] = (ev, ef[:n], 1.0, polar(9.0, 31.0))
    out["empty"] = (ev, ef[:0], 1.0, polar(9.0, 31.0))
    out["above"] = (ev, ef, 1.0, polar(6.0, -75.0, z=4.0))                       # wholly above the 13.45 degree top row
    out["duplicate"] = (ev, np.concatenate([ef[:40], ef[10:30], ef[40:]]), 1.0, polar(9.0, 140.0))   # exact ties between copies of a face
    zero = np.array([[0, 0, 5], [1, 3, 3]], np.int32)                              # a repeated vertex
    vline = np.concatenate([ev, [ev[0] * 0.5 + ev[1] * 0.5]])                      # ... and three vertices on one line (the exact midpoint)
    out["zero_area"] = (vline, np.concatenate([zero, [[0, 1, len(ev)]], ef]), 1.0, polar(9.0, -120.0))
    # faces edge-on to the sensor: one in a vertical plane through the z axis (every ray of that column lies in it), one in a tilted plane
    # through the origin that holds the ray (row 40, column 2600) along one of its edges
    dx, dy, dz = S.sensor_tables()
    d = np.array([dx[2600], dy[2600], dz[40]]) / 120.0
    e = np.array([dx[2590], dy[2590], 0.0]) / 120.0
    vert = [8.0 * e + [0, 0, -1], 10.0 * e + [0, 0, -1], 9.0 * e + [0, 0, 1]]
    tilt = [8.0 * d, 10.0 * d, 9.0 * d + [0.3, -0.2, 0.4]]
    back = [[4.0, 11.0, -3.0], [9.0, 11.0, -3.0], [6.0, 12.0, 3.0]]              # an ordinary face behind both
    out["edge_on"] = (np.array(vert + tilt + back), np.arange(9, dtype=np.int32).reshape(3, 3), 1.0, (0.0, 0.0, 0.0, 0.0))
    return out


CASES = {
    "ellipsoid80_12m": (*ellipsoid(1), 1.0, polar(12.0, 57.0)),
    "ellipsoid80_20m": (*ellipsoid(1), 1.0, polar(20.0, -133.0, yaw=1.1)),
    "ellipsoid320_12m": (*ellipsoid(2), 1.0, polar(12.0, 57.0)),
    "ellipsoid320_20m": (*ellipsoid(2), 1.0, polar(20.0, -133.0, yaw=1.1)),
    "car_6m": (*car(), 6.0, polar(6.0, 100.0, yaw=0.7)),
    "wrap_plus180": (*ellipsoid(1), 1.0, polar(12.0, 180.0)),
    "wrap_minus180": (*ellipsoid(1), 1.0, polar(12.0, -180.0, yaw=-0.4)),
    "over_sensor": (*ellipsoid(1), 1.0, (0.3, 0.2, 0.0, 0.5)),
    **_edge_cases(),
}
CAST_CASES = ("ellipsoid80_12m", "ellipsoid80_20m", "ellipsoid320_12m", "ellipsoid320_20m", "car_6m")
EDGE_CASES = ("first1", "first63", "first64", "first65", "empty", "above", "duplicate", "zero_area", "edge_on")
WRAP_CASES = ("wrap_plus180", "wrap_minus180", "over_sensor")


@functools.lru_cache(None)
def reference(name):
    """The restatement's cloud of a case on its own window (scene_ref.cloud, noise off)."""
    v, f, scale, pose = CASES[name]
    return R.cloud(v, f, scale, pose, tables=S.sensor_tables())


# the heterogeneous batch of the generate / noise / install tests: (mesh name, scale, pose of cloud 1, pose of cloud 2, scene id)
BATCH_MESHES = {"car": car, "person": person, "ellipsoid80": lambda: ellipsoid(1)}
BATCH = (
    ("car", 4.4, polar(14.0, 20.0, yaw=1.5), polar(14.3, 22.0, yaw=1.8), 11),
    ("person", 1.8, polar(7.0, -60.0, yaw=0.2), polar(7.4, -58.0, yaw=0.5), 12),
    ("ellipsoid80", 1.0, polar(18.0, 179.5, yaw=0.9), polar(6.0, -75.0, z=4.0), 13),      # cloud 1 wraps, cloud 2 is empty (above the field of view)
    ("car", 4.4, polar(19.0, -150.0, yaw=-2.0), polar(18.5, -149.0, yaw=-2.2), 14),       # shares its mesh with scene 0
    ("ellipsoid80", 0.5, polar(5.0, 91.3, yaw=0.15), polar(5.2, 93.0, yaw=0.3), 2 ** 40 + 5),
)


@functools.lru_cache(None)
def batch_reference(k, sigma=0.0, seed=0):
    """(cloud 1, cloud 2) of scene k of BATCH by the restatement."""
    name, scale, p1, p2, sid = BATCH[k]
    v, f = BATCH_MESHES[name]()
    return tuple(R.cloud(v, f, scale, p, tables=S.sensor_tables(), seed=seed, scene_id=sid, which=w, sigma=sigma) for w, p in enumerate((p1, p2)))
