"""The clouds and parameter sets that tests/test_goicp_cpu.py and tests/test_goicp_gpu.py share.  Small on purpose (|S| <= 64, |Q| <= 200,
frontier <= 2^16, coarse resolutions): the restatement evaluates every node in NumPy."""
import functools

import numpy as np

from tests import goicp_ref as G


def car(n, seed, noise=0.0):
    """n points on a car-like shell: a 4.0 x 1.8 x 0.7 body with a 1.9 x 1.5 x 0.5 cabin set 0.35 m to the rear -- close to its own mirror
    image under a half turn, which is what sends a local method into the wrong basin."""
    rng = np.random.RandomState(seed)
    pts = np.empty((n, 3))
    for i in range(n):
        if rng.rand() < 0.65:
            c, e = np.array([0.0, 0.0, 0.35]), np.array([2.0, 0.9, 0.35])
        else:
            c, e = np.array([-0.35, 0.0, 0.95]), np.array([0.95, 0.75, 0.25])
        u = rng.uniform(-1.0, 1.0, 3)
        k = rng.randint(5)   # four sides and the roof
        if k < 2:
            u[0] = 1.0 if k == 0 else -1.0
        elif k < 4:
            u[1] = 1.0 if k == 2 else -1.0
        else:
            u[2] = 1.0
        pts[i] = c + e * u
    return pts + noise * rng.randn(n, 3)


def rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def planted(n1, n2, seed, yaw, t, noise=0.003, origin=(0.0, 0.0, 0.0)):
    """(source [n1, 3], target [n2, 3]) float32: the target is the posed source's shell (its first n1 points the source's own, moved) plus
    noise, both in a frame at `origin`."""
    shell = car(max(n1, n2), seed)
    rng = np.random.RandomState(seed + 1000)
    src = shell[:n1] + np.asarray(origin)
    tgt = shell[:n2] @ rz(yaw).T + np.asarray(t) + noise * rng.randn(n2, 3) + np.asarray(origin)
    return src.astype(np.float32), tgt.astype(np.float32)


def symmetric(n, seed):
    """A cloud that a half turn about its centre maps onto itself: every optimum comes twice."""
    half = car(n // 2, seed)
    half = half - half.mean(0)
    both = np.concatenate([half, half * np.array([-1.0, -1.0, 1.0])], 0)
    return both.astype(np.float32)


COARSE = dict(yaw_res=np.pi / 128, t_half=(0.4, 0.4, 0.0), t_res=0.06, trunc=0.5, mse_thresh=1e-4, max_source=64, max_target=200,
              max_frontier=1 << 16, starts=0)
COARSER = dict(COARSE, yaw_res=np.pi / 32, t_res=0.12)

YAW_170 = np.deg2rad(170.0)


# name -> (source, target, parameter overrides); "symmetric" is the one case whose decision margins are not asserted
@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    s, t = planted(48, 150, 11, YAW_170, (0.12, -0.07, 0.0))
    out["planted170"] = (s, t, dict(COARSE))
    out["certified"] = (s, t, dict(COARSE, mse_thresh=1e-2))
    s, t = planted(64, 200, 23, np.deg2rad(-35.0), (0.05, 0.21, 0.0), noise=0.02)
    out["noisy"] = (s, t, dict(COARSER, mse_thresh=1e-6))
    s, t = planted(40, 120, 5, np.deg2rad(100.0), (-0.1, 0.1, 0.05), noise=0.004)
    out["starts_z"] = (s, t, dict(COARSER, t_half=(0.4, 0.4, 0.1), starts=4, start_radius=0.3, mse_thresh=1e-5))
    s, t = planted(33, 65, 7, np.deg2rad(60.0), (0.0, 0.0, 0.0), noise=0.01)
    out["overflow"] = (s, t, dict(COARSER, max_frontier=40, mse_thresh=1e-7))
    out["levels"] = (s, t, dict(COARSER, max_levels=2, mse_thresh=1e-7))
    s, t = planted(64, 200, 31, np.deg2rad(20.0), (0.1, 0.0, 0.0), noise=0.003, origin=(3000.0, -4000.0, 12.0))
    out["far5km"] = (s, t, dict(COARSER, yaw_half=np.pi / 2))
    sym = symmetric(64, 3)
    out["symmetric"] = (sym, (sym.astype(np.float64) @ rz(np.deg2rad(40.0)).T).astype(np.float32), dict(COARSER))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's result of a case with the margins of its decisions: computed once, shared, never modified."""
    s, t, kw = cases()[name]
    margins = []
    res = G.search(s, t, G.params(**kw), margins=margins)
    res["margins"] = np.asarray(margins, np.float64)
    return res
