"""CPU: the Go-ICP restatement (tests/goicp_ref.py) that defines csrc/alignnet_goicp.hip -- its bounds are bounds, its lower bound is a
certificate, it finds the planted pose a local method misses, and none of the decisions the GPU tests compare exactly is a near-tie --
plus the surface the feature adds (struct, symbols, script)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from alignnet3d import _capi
from oracle import icp_ref
from tests import goicp_cases as K
from tests import goicp_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")
ASSERTED = [n for n in K.cases() if n != "symmetric"]


def _problem(name):
    s, t, kw = K.cases()[name]
    p = G.params(**kw)
    return G.Problem(s, t, p), p


def _schedule(pr, p):
    """The depths of every level the search can reach."""
    depth, out = np.zeros(4, np.int64), []
    for _ in range(p["max_levels"]):
        out.append(depth.copy())
        split = pr.widths(depth) > pr.res
        if not split.any():
            break
        depth = depth + split
    return out


@pytest.mark.parametrize("name", ["planted170", "starts_z"])
def test_bounds_are_valid_at_every_level(name):
    """lb <= E at 200 poses sampled inside the node and ub = E(centre), for nodes of every level: the root (delta = pi), the levels where only
    yaw is still halved, and (planted170) the zero-width z dimension.  The slack 1e-12 E is the rounding of two 64-term sums."""
    pr, p = _problem(name)
    rng = np.random.RandomState(1)
    for depth in _schedule(pr, p):
        w = pr.widths(depth)
        coords = np.stack([rng.randint(0, 1 << d, 3) for d in depth], 1)
        ub, lb = pr.bounds(depth, coords)
        centres = pr.centres(depth, coords)
        for k in range(len(coords)):
            assert ub[k] == pr.energies(centres[k:k + 1])[0]
            poses = centres[k] + rng.uniform(-1.0, 1.0, (200, 4)) * w
            poses[:3] = centres[k] + np.array([[1, 1, 1, 1], [-1, -1, -1, -1], [1, -1, 1, -1]]) * w   # corners too
            E = pr.energies(poses)
            assert np.all(lb[k] <= E * (1 + 1e-12)), (depth, coords[k], lb[k], E.min())
            assert lb[k] <= ub[k]


@pytest.mark.parametrize("name", ["planted170", "certified", "starts_z", "far5km", "symmetric"])
def test_lower_bound_is_a_certificate(name):
    """No pose of the domain has E below lower_bound - 1e-9, on the lattice of the leaves' centres and at 1500 poses drawn inside the domain;
    and error <= lattice minimum + eps: a leaf was either evaluated (E >= error) or lies in a box pruned with lb >= best - eps >= error - eps.
    (A lattice finer than the leaves could undercut `error` by more than eps at a RESOLUTION stop: the leaf lattice is the grid that the claim
    is about.)  For the symmetric cloud this and `error` below are all that is checked."""
    pr, p = _problem(name)
    res = K.reference(name)
    assert res["status"] in (G.CERTIFIED, G.RESOLUTION)
    depth = _schedule(pr, p)[-1]
    axes = [pr.centres(depth, np.stack([np.arange(1 << depth[k])] * 4, 1))[:, k] for k in range(4)]
    lattice = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 4)
    E = pr.energies(lattice)
    assert E.min() >= res["lower_bound"] - 1e-9
    assert res["error"] <= E.min() + pr.eps
    rng = np.random.RandomState(2)
    E2 = pr.energies(rng.uniform(-1.0, 1.0, (1500, 4)) * pr.half)
    assert E2.min() >= res["lower_bound"] - 1e-9
    assert res["error"] == pr.energy(res["pose"][0], res["pose"][1:])
    assert res["lower_bound"] <= res["error"] - pr.eps


def test_planted_half_turn_is_recovered_where_icp_from_the_centroid_is_not():
    s, t, kw = K.cases()["planted170"]
    res = K.reference("planted170")
    yaw = np.arctan2(res["transform"][1, 0], res["transform"][0, 0])
    err = abs((yaw - K.YAW_170 + np.pi) % (2 * np.pi) - np.pi)
    assert err <= 2 * kw["yaw_res"], np.rad2deg(err)   # the best centre is within a leaf or two of the truth
    assert res["fitness"] == 1.0
    init = np.eye(4)
    init[:3, 3] = t.astype(np.float64).mean(0) - s.astype(np.float64).mean(0)
    T, _, _, _ = icp_ref.icp_p2point_z(s, t, init, 0.1, 30)
    icp_err = abs((np.arctan2(T[1, 0], T[0, 0]) - K.YAW_170 + np.pi) % (2 * np.pi) - np.pi)
    assert icp_err > np.pi / 2, np.rad2deg(icp_err)   # the wrong basin: the near-mirror pose


@pytest.mark.parametrize("name", ASSERTED)
def test_no_decision_is_a_near_tie(name):
    """The GPU tests compare per-level counts exactly: no prune test (lb against best - eps) and no best-pose comparison of the restatement
    may lie within 1e-7 relative of its threshold, so that rounding of the order 1e-12 cannot flip one."""
    m = K.reference(name)["margins"]
    assert len(m) and np.nanmin(m) >= 1e-7, np.nanmin(m)


def test_statuses_and_empty():
    assert {K.reference(n)["status"] for n in K.cases()} == {G.CERTIFIED, G.RESOLUTION, G.OVERFLOW, G.LEVELS}
    s, _, kw = K.cases()["levels"]
    res = G.search(s, np.zeros((0, 3), np.float32), G.params(**kw))
    assert res["status"] == G.EMPTY and res["error"] == 0.0 and np.array_equal(res["transform"], np.eye(4)) and res["evaluated"].sum() == 0
    ov = K.reference("overflow")
    assert ov["survived"][1] * 8 > 40 and ov["evaluated"][2] == 0
    assert K.reference("levels")["evaluated"][2] == 0


def test_children_order_and_working_sets():
    c = G.children([[1, 2, 3, 0]], [True, False, True, False])
    assert c.tolist() == [[2, 2, 6, 0], [2, 2, 7, 0], [3, 2, 6, 0], [3, 2, 7, 0]]
    pts = np.arange(30, dtype=np.float32).reshape(10, 3)
    assert np.array_equal(G.working_set(pts, 4), pts[[0, 2, 5, 7]]) and G.working_set(pts, 10) is not None and len(G.working_set(pts, 12)) == 10


def test_surface_struct_symbols_and_defaults():
    text = open(os.path.join(ROOT, "include", "alignnet_hip.h")).read()
    for name in ("alignnet_goicp_register", "alignnet_goicp_register_dataset", "alignnet_debug_goicp_nodes"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _capi.SYMBOLS
    assert C.sizeof(_capi.GoicpParams) == 10 * 8 + 8 * 4
    fields = re.search(r"typedef struct \{([^}]*)\} alignnet_goicp_params;", text).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.split("[")[0] for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", fields) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [f[0] for f in _capi.GoicpParams._fields_]
    assert int(re.search(r"#define ALIGNNET_GOICP_MAX_LEVELS (\d+)", text).group(1)) == _capi.GOICP_MAX_LEVELS == G.MAX_LEVELS
    for k, name in enumerate(G.STATUS_NAMES):
        assert re.search(r"#define ALIGNNET_GOICP_%s %d\b" % (name, k), text)
    from alignnet3d.engine import Engine
    assert Engine.GOICP_STATUS == G.STATUS_NAMES
    assert set(Engine.GOICP_DEFAULTS) == set(G.DEFAULTS)
    for k, v in G.DEFAULTS.items():
        assert np.all(np.asarray(Engine.GOICP_DEFAULTS[k]) == np.asarray(v)), k
    with pytest.raises(NotImplementedError):
        Engine._goicp_params(False, None, {})
    with pytest.raises(ValueError):
        Engine._goicp_params(True, "p2plane", {})
    with pytest.raises(TypeError):
        Engine._goicp_params(True, None, {"yaw": 1})


def test_icp_goicp_refuses_other_configs(tmp_path):
    root = tmp_path / "D"
    os.makedirs(root / "split")
    for f in ("train.txt", "val.txt"):
        open(root / "split" / f, "w").write("0\n")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    for name, special in (("icp_D_o3_gicp", {"mode": "icp", "icp": {"variant": "o3_gicp", "with_constraint": True}}),
                          ("icp_D_goicp_p2plane", {"mode": "icp", "icp": {"variant": "goicp", "with_constraint": True, "refine": "p2plane"}}),
                          ("icp_D_goicp_free", {"mode": "icp", "icp": {"variant": "goicp", "with_constraint": False}})):
        p = tmp_path / (name + ".json")
        json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")}, "evaluation": {"special": special}}, open(p, "w"))
        r = subprocess.run([sys.executable, os.path.join(PKG, "icp_goicp.py"), "--config", str(p)], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "icp_goicp.py accepts" in r.stderr and "goicp" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(tmp_path / "logs"), "nothing is written for a config it refuses"
