"""CPU: the definition of the evaluation call (tests/reg_eval_ref.py) against hand-computed cases, the committed inputs of the GPU tests (no
undecided point on any of them), and the C header / ctypes table / Engine wrapper of alignnet_evaluate_registration*."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import alignnet3d
from alignnet3d import _capi
from tests import reg_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alignnet_evaluate_registration", "alignnet_evaluate_registration_dataset")


def test_distance_exactly_the_threshold_is_an_inlier():
    r = R.evaluate_registration([[0.0, 0.0, 0.0]], [[0.125, 0.0, 0.0]], np.eye(4), 0.125, exact=True)
    assert r["fitness"] == 1.0 and r["rmse"] == 0.125 and r["correspondences"].tolist() == [0]
    r = R.evaluate_registration([[0.0, 0.0, 0.0]], [[np.nextafter(np.float32(0.125), np.float32(1))], [0.0], [0.0]], np.eye(4), 0.125, exact=True)
    assert r["fitness"] == 0.0 and r["rmse"] == 0.0 and r["correspondences"].tolist() == [-1] and not r["information"].any()


def test_exact_tie_goes_to_the_lower_index():
    dst = [[9.0, 9.0, 9.0], [0.5, 0.0, 0.0], [-0.5, 0.0, 0.0]]
    r = R.evaluate_registration([[0.0, 0.0, 0.0]], dst, np.eye(4), 1.0, exact=True)
    assert r["correspondences"].tolist() == [1] and r["rmse"] == 0.5
    r = R.evaluate_registration([[0.0, 0.0, 0.0]], dst[::-1], np.eye(4), 1.0, exact=True)
    assert r["correspondences"].tolist() == [0]


def test_single_inlier_information_matrix_by_hand():
    # target (1, 2, 3): G = [0, 3, -2, 1, 0, 0; -3, 0, 1, 0, 1, 0; 2, -1, 0, 0, 0, 1]
    want = np.array([[13.0, -2.0, -3.0, 0.0, -3.0, 2.0],
                     [-2.0, 10.0, -6.0, 3.0, 0.0, -1.0],
                     [-3.0, -6.0, 5.0, -2.0, 1.0, 0.0],
                     [0.0, 3.0, -2.0, 1.0, 0.0, 0.0],
                     [-3.0, 0.0, 1.0, 0.0, 1.0, 0.0],
                     [2.0, -1.0, 0.0, 0.0, 0.0, 1.0]])
    T = np.eye(4)
    T[:3, 3] = [1.0, 2.0, 2.75]   # the source at the origin lands 0.25 under the target; a second source lands far away
    r = R.evaluate_registration([[0.0, 0.0, 0.0], [50.0, 0.0, 0.0]], [[1.0, 2.0, 3.0]], T, 0.5, exact=True)
    assert r["fitness"] == 0.5 and r["rmse"] == 0.25 and r["correspondences"].tolist() == [0, -1]
    assert np.array_equal(r["information"], want)


def test_centre_on_the_target_leaves_only_the_translation_block():
    T = np.eye(4)
    r = R.evaluate_registration([[1.0, 2.0, 3.0]] * 3, [[1.0, 2.0, 3.0]], T, 0.5, centre=[1.0, 2.0, 3.0], exact=True)
    want = np.zeros((6, 6))
    want[3:, 3:] = 3.0 * np.eye(3)
    assert r["fitness"] == 1.0 and r["rmse"] == 0.0 and np.array_equal(r["information"], want)


def test_empty_clouds():
    for n1, n2 in ((0, 4), (4, 0), (0, 0)):
        r = R.evaluate_registration(np.zeros((n1, 3)), np.ones((n2, 3)), np.eye(4), 0.1)
        assert r["fitness"] == 0.0 and r["rmse"] == 0.0 and r["correspondences"].tolist() == [-1] * n1 and not r["information"].any()


def test_committed_inputs_have_no_undecided_point_and_reach_their_edges():
    cases = R.all_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    res = {c["name"]: R.evaluate_registration(c["src"], c["dst"], c["T"], c["threshold"], c["centre"], c["exact"]) for c in cases}
    for name, r in res.items():
        assert not r["undecided"].any(), name
        assert np.array_equal(r["information"], r["information"].T), name
    # the target behind the scan's LDS stage is somebody's correspondence
    assert res["size_257_%d" % (R.LDS_BUDGET + 1)]["correspondences"][0] == R.LDS_BUDGET
    # threshold edge: on and inside are inliers at their exact distances, outside is not
    case, per = R.threshold_edge_case()
    r = res["threshold_edge"]
    assert (r["correspondences"][:2 * per] >= 0).all() and (r["correspondences"][2 * per:] == -1).all() and r["fitness"] == 2.0 / 3.0
    assert (r["dist2"][:per] == case["threshold"] ** 2).all() and (r["dist2"][per:2 * per] < case["threshold"] ** 2).all()
    # ties: every source has FOUR targets at its smallest distance and takes the lowest index of them
    case = R.tie_case()
    d2 = ((case["src"].astype(np.float64)[:, None] - case["dst"].astype(np.float64)[None]) ** 2).sum(-1)
    assert ((d2 == d2.min(1, keepdims=True)).sum(1) == 4).all()
    assert np.array_equal(res["ties4"]["correspondences"], d2.argmin(1)) and res["ties4"]["fitness"] == 1.0
    # the threshold range moves the fitness from (almost) nothing to everything
    fits = [res["threshold_%g" % t]["fitness"] for t in R.THRESHOLDS]
    assert fits == sorted(fits) and fits[0] < 0.05 and 0.2 < fits[1] < 0.95 and fits[-1] == 1.0
    # the far pair really is far, and its matrix is dominated by the lever arm unless centred
    far, cen = res["far_origin"]["information"], res["far_centred"]["information"]
    assert far.diagonal().max() > 1e9 and cen.diagonal().max() < 1e4 and res["far_origin"]["fitness"] > 0.5
    sizes = [(len(c["src"]), len(c["dst"])) for c in R.batch_cases()]
    assert len(sizes) == R.BATCH_PAIRS and any(a == 0 and b > 0 for a, b in sizes) and any(b == 0 and a > 0 for a, b in sizes)


def test_header_capi_and_late_symbols_agree():
    text = open(os.path.join(ROOT, "include", "alignnet_hip.h")).read()
    assert re.search(r"#define\s+ALIGNNET_ABI_VERSION\s+1\b", text) and _capi.ABI_VERSION == 1
    P = ctypes.POINTER
    tail = ["const double* transforms", "double threshold", "const double* centers", "double* fitness", "double* rmse", "double* information",
            "int32_t* correspondences"]
    ctail = [P(ctypes.c_double), ctypes.c_double, P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_int32)]
    head = {NAMES[0]: (["alignnet_handle* h", "const float* points1", "const float* points2", "const int64_t* offsets", "int32_t B"],
                       [P(ctypes.c_float), P(ctypes.c_float), P(ctypes.c_int64), ctypes.c_int32]),
            NAMES[1]: (["alignnet_handle* h", "const int32_t* rows", "int32_t B"], [P(ctypes.c_int32), ctypes.c_int32])}
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name + " not declared"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == head[name][0] + tail
        res, bound = _capi.SYMBOLS[name]
        assert res is ctypes.c_int and bound[1:] == head[name][1] + ctail
        assert name in _capi.LATE_SYMBOLS


def test_built_library_exports_the_symbols():
    lib = alignnet3d.load_library()
    for name in NAMES:
        assert hasattr(lib, name), "not exported by " + alignnet3d.library_path()
        assert getattr(lib, name).argtypes == _capi.SYMBOLS[name][1]


def test_library_without_the_symbols_raises_engine_error():
    eng = object.__new__(alignnet3d.Engine)
    eng._lib, eng._h, eng._dataset_sizes = types.SimpleNamespace(), None, None
    with pytest.raises(alignnet3d.EngineError, match=NAMES[0] + ".*rebuild"):
        eng.evaluate_registration([np.zeros((3, 3))], [np.zeros((3, 3))], [np.eye(4)])
    with pytest.raises(alignnet3d.EngineError, match=NAMES[1] + ".*rebuild"):
        eng.evaluate_registration_rows([0], [np.eye(4)])
