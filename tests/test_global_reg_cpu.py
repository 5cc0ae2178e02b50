"""CPU: the restatement of the global registration (tests/global_reg_ref.py: FPFH + RANSAC, the reference's o3_gicp baseline) on its own --
the generator's vectors, planted motions recovered, and the check that the skip caps of tests/test_global_reg_gpu.py hide nothing: on every
input set the GPU tests use, the restatement alone finds at most a tenth of the cap of undecided entries per stage, and no undecided
RANSAC pair.  Plus the new symbols' header / ctypes agreement and the icp_global.py command's refusal of configs it does not accept."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import global_reg_ref as G
from tests import icp_full_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")


def test_generator_vectors():
    # (seed, stream, it, k, n) -> index; from an arbitrary-precision integer evaluation of the definition
    vectors = [((0, 0, 0, 0, 1000), 0), ((0, 0, 0, 1, 1000), 338), ((0, 0, 1, 0, 1000), 717), ((0, 5, 123456, 3, 2477), 698),
               ((7, 41, 3999999, 2, 3460), 1841), ((9223372036854788153, 16777215, 274877906943, 3, 65536), 48862), ((1, 0, 0, 0, 1), 0)]
    for (seed, stream, it, k, n), want in vectors:
        assert int(G.draw(seed, stream, np.array([it]), k, n)[0]) == want
    its = np.arange(5000)
    d = np.stack([G.draw(3, 2, its, k, 977) for k in range(4)], 1)
    assert d.min() >= 0 and d.max() < 977 and len(np.unique(d)) > 900
    assert not np.array_equal(d, np.stack([G.draw(3, 3, its, k, 977) for k in range(4)], 1))
    with pytest.raises(AssertionError):
        G.draw(0, 1 << 24, its, 0, 10)


# Measured with this restatement: 6 of 6 pairs.  Clouds at car size: 4500 points on the surface of the car-sized object, 1 cm of
# clipped noise, the source an exact 70 % subset under a yaw anywhere in (-pi, pi] and up to 0.6 m of shift; downsampled sizes about 2900 and
# 4000; RANSAC capped at 200,000 iterations (110 - 190 of the 500 validations reached), then the z-constrained point-to-point ICP restatement
# (radius 0.10, 30 iterations) from its result.  Since the source is an exact subset, ICP from a start inside the basin ends on the truth to
# float32 rounding of the clouds: every pair came back with yaw and translation errors below 2e-8, under the 1e-6 bar of the ICP tests.
RECOVERED_SHARE = 6 / 6


def test_ransac_then_icp_recovers_planted_motions():
    src, dst, truth = G.car_pairs(6, seed=51)
    good = 0
    for k in range(6):
        r = G.global_register(src[k], dst[k], True, 0, k, 200000, 500)
        T = F.icp_p2point(src[k], dst[k], r["T"], 0.1, 30, with_constraint=True)[0]
        E = np.linalg.inv(truth[k]) @ T
        c = src[k].astype(np.float64).mean(0)
        yaw, shift = abs(np.arctan2(E[1, 0], E[0, 0])), np.linalg.norm(E[:3, :3] @ c + E[:3, 3] - c)
        print("pair %d: RANSAC fitness %.3f rmse %.4f validations %d; after ICP yaw error %.2e, translation error at the centroid %.2e"
              % (k, r["fitness"], r["rmse"], r["validations"], yaw, shift))
        good += yaw < 1e-6 and shift < 1e-6
    assert good / 6 >= RECOVERED_SHARE


def _shares(runs):
    """Aggregate share of undecided entries per stage over runs of global_register, and the smallest RANSAC margin."""
    tot = {}
    for r in runs:
        for side in r["stages"]:
            n = len(side["ds"]["points"])
            for stage, und in (("voxel", side["ds"]["margin"] < G.UNDECIDED),
                               ("normals", (side["normals"]["nbr_margin"] < G.UNDECIDED) | (side["normals"]["gap"] < G.UNDECIDED_GAP) | (side["normals"]["nz"] < G.UNDECIDED)),
                               ("spfh", (side["spfh"]["nbr_margin"] < G.UNDECIDED) | (side["spfh"]["margin"] < G.UNDECIDED)),
                               ("fpfh", side["fpfh"]["nbr_margin"] < G.UNDECIDED)):
                t = tot.setdefault(stage, [0, 0]); t[0] += int(und.sum()); t[1] += und.size
        t = tot.setdefault("matches", [0, 0]); t[0] += int((r["match_margin"] < G.UNDECIDED).sum()); t[1] += r["match_margin"].size
    return {k: v[0] / max(v[1], 1) for k, v in tot.items()}, min(r["margin"] for r in runs)


@pytest.mark.parametrize("constrained", [True, False])
def test_gpu_test_inputs_are_decided(constrained):
    src, dst, _ = G.gpu_test_pairs(constrained)
    runs = [G.global_register(src[k], dst[k], constrained, 3, k, G.TEST_ITERATIONS, G.TEST_VALIDATIONS) for k in range(len(src))]
    shares, margin = _shares(runs)
    print(shares, margin)
    assert all(v <= G.SKIP_CAP / 10 for v in shares.values()), shares
    assert margin >= G.UNDECIDED_RANSAC           # no undecided pair among the 8
    assert all(r["fitness"] > 0.9 and r["validations"] == G.TEST_VALIDATIONS for r in runs)


def test_gpu_single_pair_inputs_are_decided():
    s, d, _ = G.default_pair()
    r = G.global_register(s, d, True, 0, 5)
    assert r["validations"] == 500 and r["iterations"] < 4000000 and r["fitness"] > 0.95
    assert G.Ransac(r["stages"][0]["ds"]["points"], r["stages"][1]["ds"]["points"], r["matches"], True, 0, 5).run(40, 500)["validations"] == 0
    s2, d2, _ = G.large_pair()
    r2 = G.global_register(s2, d2, True, 1, 9, 100000, 20)
    assert len(r2["stages"][1]["ds"]["points"]) > 6314
    for r in (r, r2):
        shares, margin = _shares([r])
        assert all(v <= G.SKIP_CAP / 10 for v in shares.values()), shares
        assert margin >= G.UNDECIDED_RANSAC


def test_restatement_edge_cases():
    empty = np.zeros((0, 3), np.float32)
    src, dst, _ = G.car_pairs(1, seed=5, n_points=600, scale=0.2)
    for a, b in ((empty, dst[0]), (src[0], empty), (src[0][:3], dst[0])):
        r = G.global_register(a, b, True, 0, 0, 1000, 10)
        assert np.array_equal(r["T"], np.eye(4)) and (r["fitness"], r["rmse"], r["iterations"], r["validations"], r["win"]) == (0.0, 0.0, 0, 0, -1)
    # more than max_nn points within the radius: the nearest max_nn, ordered by (distance, index)
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 0.2, (300, 3))
    I, J, D, count, margin = G.neighbours(pts, 0.25, 100)
    assert count.max() == 100
    d0 = ((pts - pts[0]) ** 2).sum(1)
    assert set(J[I == 0]) == set(np.argsort(d0, kind="stable")[:100])


def test_new_symbols_declared_and_bound():
    from alignnet3d import _capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alignnet_hip.h")).read(), flags=re.S)
    for name, nargs in (("alignnet_global_register", 15), ("alignnet_global_register_dataset", 13), ("alignnet_debug_global_stages", 25)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, name + " not declared in include/alignnet_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_capi.SYMBOLS[name][1]), name
    import alignnet3d
    lib = alignnet3d.load_library()
    for name in ("alignnet_global_register", "alignnet_global_register_dataset", "alignnet_debug_global_stages"):
        assert hasattr(lib, name)
    for method in ("global_register", "global_register_rows", "debug_global_stages"):
        assert callable(getattr(alignnet3d.Engine, method))


def test_icp_global_refuses_other_configs(tmp_path):
    root = tmp_path / "D"
    os.makedirs(root / "split")
    for f in ("train.txt", "val.txt"):
        open(root / "split" / f, "w").write("0\n")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    for name, special in (("icp_D_o3_gicp_p2p", {"mode": "icp", "icp": {"variant": "o3_gicp", "with_constraint": True, "refine": "p2p"}}),
                          ("icp_D_o3_gicp_fast", {"mode": "icp", "icp": {"variant": "o3_gicp_fast", "with_constraint": True}}),
                          ("icp_D_o3_p2p", {"mode": "icp", "icp": {"variant": "p2point", "with_constraint": True}}),
                          ("held_D", {"mode": "held", "held": {"model": "x"}})):
        p = tmp_path / (name + ".json")
        json.dump({"data": {"basepath": str(root)}, "logging": {"basedir": str(tmp_path / "logs")}, "evaluation": {"special": special}}, open(p, "w"))
        r = subprocess.run([sys.executable, os.path.join(PKG, "icp_global.py"), "--config", str(p)], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "icp_global.py accepts" in r.stderr and "o3_gicp" in r.stderr, r.stderr[-2000:]
        assert not os.path.exists(tmp_path / "logs"), "nothing is written for a config it refuses"
