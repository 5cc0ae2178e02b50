"""GPU: the loss kernels alone (loss_prep_kernel, loss_pairs_body, loss_final_kernel, with stage2_finish_kernel's decode in front and
dbg_angle_class_kernel behind) through alignnet_debug_loss, against the oracle (tests/loss_ref.py) on the cases of tests/loss_cases.py: every
batch size at which the launch shape changes (1, 2, 3, 63, 64, 65, 129, 1025), bin counts on both sides of the 16-lane and 64-lane trips (1 .. 130), both
settings of accept_inverted, three factor pairs; labels on the wrap, far out, equal, and a sweep of every bin boundary +-3 float32 steps for the classes.

Bars (measured on the oracle alone, float32 against float64 evaluation of the same graph; tests/loss_ref.py bars(), asserted in tests/test_loss_cpu.py):
    u_v = 1.47e-5 (values), u_g = 7.4e-8 (d_s1c), 1.1e-7 (d_s2c), 3.9e-5 (d_o2), 3.9e-5 (d_o3); a result passes at 4 u, and never above 1e-4.
Measured worst errors of the kernels on an MI355X over the 22 value cases (printed by test_values_and_gradients):
    values 2.49e-5 (bar 5.9e-5), d_s1c 6.0e-8 (3.0e-7), d_s2c 9.9e-8 (4.5e-7), d_o2 3.9e-5 (1e-4), d_o3 3.9e-5 (1e-4)
-- case by case where the float32 oracle sits: the error is the residual label's (an angle of float32 step 4.8e-7 divided by pi / nb), not the summation's.
No case needed more than the margin."""
import ctypes as C

import numpy as np
import pytest

import alignnet3d
from alignnet3d import _capi
from tests import loss_cases as LC
from tests import loss_ref as LR
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(), device=0)   # its own num_bins (12) and factors enter nothing: every case passes its own
    yield e
    e.close()


def run(eng, case, want_grad=True, want_classes=True):
    return eng.debug_loss(case["o2"], case["s1c"], case["o3"], case["labels"], case["nb"], case["accept_inverted"], case["esf"], case["af"],
                          want_grad=want_grad, want_classes=want_classes)


@pytest.fixture(scope="module")
def results(eng):
    """every value case once, with gradient and classes"""
    return {c: run(eng, LR.reference(c)["case"]) for c in LC.VALUE_CASES}


def test_decode(results):
    """theta, pcls against R.get_angles in float32 (pcls exact: ties -- the first maximum wins -- and nb = 65, 130, the arg-max's second trip; theta to
    2 ulps of pi), s2c == o2[:, :3] + s1c bit for bit."""
    seen_tie = 0
    for c in LC.VALUE_CASES:
        r, res = LR.reference(c), results[c]
        case, v32 = r["case"], r["v32"]
        assert np.array_equal(res["pcls"], v32["pcls"]), LC.case_id(c)
        lg = case["o2"][:, 3:3 + case["nb"]]
        seen_tie += int(((lg == lg.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        d = np.abs(res["theta"].astype(np.float64) - v32["theta"].astype(np.float64)).max()
        assert d <= 2 * float(np.spacing(np.float32(np.pi))), (LC.case_id(c), d)
        assert np.abs(res["theta"]).max() <= np.float32(np.pi)
        assert np.array_equal(res["s2c"], LR.endpoints(case, np.float32)[1]), LC.case_id(c)
    assert seen_tie >= 30


def test_label_classes_of_the_value_cases(results):
    for c in LC.VALUE_CASES:
        r = LR.reference(c)
        assert not LR.judge_classes(results[c]["cls"], r["v32"]["cls"], c[1]), LC.case_id(c)


@pytest.mark.parametrize("nb", LC.BIN_COUNTS)
def test_label_classes_on_the_boundary_sweep(eng, nb):
    """Every bin boundary +-3 float32 steps, the wrap included: the classes of all three terms equal the float32 oracle's and lie in [0, nb).  nb = 17 and 19
    (test below) hold labels whose float32 quotient is nb itself: class 0 by the project's rule (before it: nb from the read-back, nb - 1 in the loss)."""
    n = 0
    for case in LC.sweep_cases(nb):
        res = run(eng, case, want_grad=False)
        ref = LR.oracle_values(case, np.float32)
        bad = LR.judge_classes(res["cls"], ref["cls"], nb)
        assert not bad, (case["id"], bad)
        n += sum(k.size for k in res["cls"])
    assert n >= 7 * (nb + 1)


def test_out_of_range_labels_wrap_to_class_0(eng):
    for nb in (17, 19):
        hit = 0
        for case in LC.sweep_cases(nb):
            res = run(eng, case, want_grad=False)
            for t, key in ((0, "pc1_angles"), (1, "pc2_angles")):
                raw = LR.kernel_class_rule(case["labels"][key][:, 0], nb, "raw")[0]
                assert np.array_equal(res["cls"][t][0], np.where(raw == nb, 0, raw))
                hit += int((raw == nb).sum())
        assert hit >= 2, (nb, hit)


def test_values_and_gradients(results):
    """out[0..16] against the float64 oracle at 4 u_v, the chosen variant per term, d_s1c / d_s2c / d_o2 / d_o3 against float64 autograd at 4 u_g per tensor,
    d_o2[:, :3] zero, every logit gradient exactly zero with angle_factor 0 (tests/loss_ref.py judge)."""
    figures, failed = {}, []
    for c in LC.VALUE_CASES:
        f = {}
        bad = LR.judge(results[c], c, f)
        print(LC.case_id(c), " ".join("%s %.3g" % kv for kv in f.items()))
        for k, v in f.items():
            figures[k] = max(figures.get(k, 0.0), v)
        for k in LR.GRAD_KEYS:
            assert np.isfinite(results[c][k]).all(), (LC.case_id(c), k)
        if bad:
            failed.append((LC.case_id(c), bad))
    u_v, u_g = LR.bars()
    print("bars: u_v %.3g" % u_v, " ".join("%s %.3g" % kv for kv in u_g.items()))
    print("kernels, worst:", " ".join("%s %.3g" % kv for kv in figures.items()))
    assert not failed, failed


def test_values_do_not_depend_on_want_grad(eng, results):
    for c in LC.VALUE_CASES[::3]:
        res = run(eng, LR.reference(c)["case"], want_grad=False, want_classes=False)
        assert res["out"].tobytes() == results[c]["out"].tobytes(), LC.case_id(c)


def test_rows_do_not_depend_on_the_launch_shape(eng, results):
    """The B = 65 case copied into rows 0 .. 64 of a B = 129 problem: theta, pcls and the classes of those rows are the same bits (per-row quantities
    depend on nothing but their row -- and, for the pair term, their column)."""
    small, big = (65, 12, True, 0.5, 1.0), (129, 12, True, 0.5, 1.0)
    cs, cb = LR.reference(small)["case"], LR.reference(big)["case"]
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cb.items()}
    case["labels"] = {k: v.copy() for k, v in cb["labels"].items()}
    for t in range(2):
        case["o2"][t * 129:t * 129 + 65] = cs["o2"][t * 65:(t + 1) * 65]
        case["s1c"][t * 129:t * 129 + 65] = cs["s1c"][t * 65:(t + 1) * 65]
    case["o3"][:65] = cs["o3"]
    for k in case["labels"]:
        case["labels"][k][:65] = cs["labels"][k]
    res, ref = run(eng, case, want_grad=False), results[small]
    for t in range(2):
        assert res["theta"][t * 129:t * 129 + 65].tobytes() == ref["theta"][t * 65:(t + 1) * 65].tobytes()
        assert np.array_equal(res["pcls"][t * 129:t * 129 + 65], ref["pcls"][t * 65:(t + 1) * 65])
        assert np.array_equal(res["s2c"][t * 129:t * 129 + 65], ref["s2c"][t * 65:(t + 1) * 65])
        assert np.array_equal(res["cls"][t][:, :65], ref["cls"][t])
    assert np.array_equal(res["cls"][2][:, :65, :65], ref["cls"][2])


def test_same_case_twice_is_bit_identical(eng, results):
    for c in ((129, 50, True, 0.1, 1.5), (1025, 12, True, 0.5, 1.0)):
        res = run(eng, LR.reference(c)["case"])
        for k in ("out", "theta", "pcls", "s2c") + LR.GRAD_KEYS:
            assert res[k].tobytes() == results[c][k].tobytes(), (LC.case_id(c), k)
        for t in range(3):
            assert np.array_equal(res["cls"][t], results[c]["cls"][t])


def test_bad_arguments_are_errors_and_launch_nothing(eng, results):
    c = LC.VALUE_CASES[5]
    case = LR.reference(c)["case"]
    keep, L = eng._labels(case["labels"], case["B"])
    fp = lambda a: a.ctypes.data_as(_capi.FP)
    out = np.full(17, 7.0, np.float32)

    def call(B, nb, labels, o2=case["o2"]):
        return eng._lib.alignnet_debug_loss(eng._h, B, nb, int(case["accept_inverted"]), case["esf"], case["af"], 0, fp(o2) if o2 is not None else None, fp(case["s1c"]), fp(case["o3"]), labels, fp(out),
                                            None, None, None, None, None, None, None, None, None, None)
    assert call(0, case["nb"], C.byref(L)) != 0 and b"B and nb" in eng._lib.alignnet_last_error(eng._h)
    assert call(-3, case["nb"], C.byref(L)) != 0
    assert call(case["B"], 0, C.byref(L)) != 0 and b"B and nb" in eng._lib.alignnet_last_error(eng._h)
    assert call(case["B"], case["nb"], None) != 0
    assert call(case["B"], case["nb"], C.byref(L), o2=None) != 0
    L2 = _capi.Labels()
    for k in LC.LABEL_KEYS:
        setattr(L2, k, getattr(L, k))
    L2.pc2_angles = None
    assert call(case["B"], case["nb"], C.byref(L2)) != 0 and b"six label tensors" in eng._lib.alignnet_last_error(eng._h)
    assert np.all(out == 7.0)   # nothing written
    assert call(case["B"], case["nb"], C.byref(L)) == 0 and out.tobytes() == results[c]["out"].tobytes()   # and the engine still works
    with pytest.raises(ValueError):
        eng.debug_loss(case["o2"][:-1], case["s1c"], case["o3"], case["labels"], case["nb"])
