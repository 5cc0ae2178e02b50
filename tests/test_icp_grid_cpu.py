"""CPU: the cell function of the ICP grid search as restated in tests/icp_grid_ref.py (csrc/alignnet_icp.hip states the same in its header comment),
the new C entry point's declaration and binding, and the drop-in's config key.  No compute calls (there is no GPU and no CPU fallback)."""
import os
import re
import sys

import numpy as np
import pytest

from alignnet3d import _capi
from tests import icp_grid_ref as G
from tests import icp_scan_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alignnet-3d_amd")


def _pairs(offset, n, seed):
    """Float32 query / target coordinates whose fp64 squared distance is <= radius^2: random directions with lengths up to the radius, and planted ones
    EXACTLY (to the float32 grid) one radius apart along an axis, in both directions, with the float32 neighbours of that."""
    rng = np.random.default_rng(seed)
    a = (rng.uniform(-20, 20, (n, 3)) + offset).astype(np.float32)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    b = (a.astype(np.float64) + u * G.RADIUS * rng.uniform(0, 1, (n, 1)) ** (1.0 / 3.0)).astype(np.float32)
    m = n // 2
    axis, sign = rng.integers(3, size=m), rng.choice([-1.0, 1.0], size=m)
    b[:m] = a[:m]
    planted = (a[np.arange(m), axis].astype(np.float64) + sign * G.RADIUS).astype(np.float32)
    toward = np.nextafter(planted, a[np.arange(m), axis])                 # one float32 step back towards the query
    b[np.arange(m), axis] = np.where(np.arange(m) % 2 == 0, planted, toward)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    d2 = (a64[:, 0] - b64[:, 0]) ** 2 + (a64[:, 1] - b64[:, 1]) ** 2 + (a64[:, 2] - b64[:, 2]) ** 2
    keep = d2 <= G.RADIUS * G.RADIUS
    return a64[keep], b64[keep]


@pytest.mark.parametrize("offset", [0.0, 4096.0])
def test_every_target_within_the_radius_lies_in_the_27_cells(offset):
    a, b = _pairs(offset, 1000000, seed=4)
    assert len(a) > 600000
    e = G.cell_edge(b, G.RADIUS)
    assert e > G.RADIUS and e == G.RADIUS * (1.0 + G.SPAN)
    span = np.abs(G.cells(a, e) - G.cells(b, e)).max(1)
    assert span.max() == 1, "a target within the radius outside the 27 cells"
    # The check can fail: cells 1 % narrower than the radius lose inliers.  Cells EXACTLY one radius wide lose none of these pairs: with this cell
    # function (no origin subtracted, one correctly rounded division) two coordinates within the radius in fp64 land two cells apart only when the
    # quotients' rounding (2^-53 relative) bridges the gap, which float32 targets next to a cell border of 0.1 do not come near.  Pairs that land two
    # cells apart at e = radius are pairs whose float32 rounding put them MORE than the radius apart (1e-6 of draws near the origin, 1e-3 at
    # 4 km; the margin does not change that, and they are no inliers).  The margin is kept for the bound in the kernel's comment, which holds for
    # every radius and magnitude, not for a loss seen here.
    narrow = np.abs(G.cells(a, 0.99 * G.RADIUS) - G.cells(b, 0.99 * G.RADIUS)).max(1) > 1
    exact = np.abs(G.cells(a, G.RADIUS) - G.cells(b, G.RADIUS)).max(1) > 1
    print("offset %s: %d pairs within the radius; two cells apart: %d with e = 0.99 radius, %d with e = radius" % (offset, len(a), narrow.sum(), exact.sum()))
    assert narrow.sum() > 100


def test_cell_edge_is_enlarged_for_small_radii_and_cells_stay_in_range():
    q = np.array([[4096.0, -3.0, 1.0], [4100.0, 2.0, 0.5]], np.float32)
    e = G.cell_edge(q, 1e-3)
    assert e == (4100.0 + 1e-3) * G.SPAN > 1e-3 and np.abs(G.cells(q, e)).max() <= 2 ** 20
    assert G.cell_edge(q, 0.1) == 0.1 * (1.0 + G.SPAN)
    assert np.array_equal(G.cells(np.array([1e300, -1e300, np.inf]), 0.1), [2 ** 30, -2 ** 30, 2 ** 30])
    # the recipe of the GPU tests: no undecided point in the first evaluation
    src, dst, T, init = G.box_pair(4267, 0.0)
    ev = S.evaluate_with_margins(src, dst, init, G.RADIUS)
    near27, within, lost = G.neighbour_counts(ev["p"], dst, G.cell_edge(dst, G.RADIUS), G.RADIUS)
    print("box 4267: fitness %.3f, %d undecided, %.1f targets in the 27 cells per query (of %d)" % (ev["fitness"], ev["undecided"].sum(), near27.mean(), len(dst)))
    assert not lost.any() and ev["undecided"].sum() <= S.POINT_CAP * len(src) and 0.5 < ev["fitness"] < 1.0 and near27.mean() < 200


def test_header_declares_and_capi_binds_the_grid_read_back():
    text = open(os.path.join(ROOT, "include", "alignnet_hip.h")).read()
    assert re.search(r"\bint alignnet_debug_icp_grid\s*\(", text) and '"icp_search"' in text
    assert "alignnet_debug_icp_grid" in _capi.SYMBOLS
    restype, argtypes = _capi.SYMBOLS["alignnet_debug_icp_grid"]
    assert len(argtypes) == 17
    assert "#define ALIGNNET_ABI_VERSION 1\n" in text and _capi.ABI_VERSION == 1


def test_train_py_icp_search_key():
    sys.path.insert(0, PKG)
    try:
        import train
        from config import NameSpace
    finally:
        sys.path.remove(PKG)

    def conf(**ev):
        c, e = NameSpace(), NameSpace()
        vars(e).update(ev)
        vars(c)["evaluation"] = e
        return c

    assert train.icp_search_option(conf(), {}) == ("scan", 0)
    for name, value in (("scan", 0), ("grid", 1), ("auto", 2)):
        assert train.icp_search_option(conf(icp_search=name), {}) == (name, value)
        assert train.icp_search_option(conf(), {"ALIGNNET_ICP_SEARCH": name}) == (name, value)
    assert train.icp_search_option(conf(icp_search="scan"), {"ALIGNNET_ICP_SEARCH": "grid"}) == ("grid", 1)
    for bad in ("kdtree", "1", "Grid "):
        with pytest.raises(ValueError, match="icp_search"):
            train.icp_search_option(conf(icp_search=bad), {})
    with pytest.raises(ValueError, match="icp_search"):
        train.icp_search_option(conf(), {"ALIGNNET_ICP_SEARCH": "fast"})
