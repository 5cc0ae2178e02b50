"""CPU: the one-call registration's definition and surface.  tests/register_ref.py restates, in NumPy, what csrc/alignnet_register.hip computes
between the network and the ICP; here that restatement is held against the host code it restates (models.tp8.classLogits2angle bit for bit,
evaluation.get_mat_angle to a few ulps), and the header, the ctypes table, the built library and train.py's option parser are checked."""
import ctypes as C
import json
import os
import re
import sys
import types

import numpy as np
import pytest

import alignnet3d
from alignnet3d import _capi
from tests import register_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "alignnet-3d_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)
G = np.load(os.path.join(HERE, "golden", "reference_vectors.npz"))


def _host_decode(monkeypatch, logits, nb):
    import models.tp8 as tp8
    monkeypatch.setattr(tp8, "cfg", types.SimpleNamespace(model=types.SimpleNamespace(angles=types.SimpleNamespace(num_bins=nb))))
    return tp8.classLogits2angle(logits)


def test_decode_equals_host_on_golden_logits(monkeypatch):
    logits = G["dec_logits"]
    nb = logits.shape[1] // 2
    got = RR.decode(logits, nb)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, G["dec_angles"])
    np.testing.assert_array_equal(got, _host_decode(monkeypatch, logits, nb))


@pytest.mark.parametrize("nb", [1, 12, 50])
def test_decode_equals_host_on_random_logits(monkeypatch, nb):
    rng = np.random.default_rng(100 + nb)
    logits = rng.normal(size=(257, 2 * nb)).astype(np.float32)
    logits[:, nb:] *= 0.3
    got = RR.decode(logits, nb)
    np.testing.assert_array_equal(got, _host_decode(monkeypatch, logits, nb))
    assert np.all(got <= np.pi)
    if nb > 1:
        assert (got < 0).any() and (got > 0).any()   # both sides of the wrap are met


def test_decode_planted_tie_pi_and_one_ulp_above(monkeypatch):
    # an exact tie between two classes: the first wins (np.argmax)
    nb = 12
    k = 2 * np.pi / nb
    logits = np.zeros((3, 2 * nb), np.float32)
    logits[0, [3, 7]] = 1.5; logits[0, nb + 3] = 0.25; logits[0, nb + 7] = -0.25
    logits[1, :nb] = 0.0; logits[1, nb] = 0.125            # every class ties: class 0
    logits[2, [11, 2]] = 2.0; logits[2, nb + 2] = 0.5; logits[2, nb + 11] = 0.1
    got = RR.decode(logits, nb)
    np.testing.assert_array_equal(got, [3 * k + 0.25, 0.125, 2 * k + 0.5])
    np.testing.assert_array_equal(got, _host_decode(monkeypatch, logits, nb))
    # an angle exactly pi stays; one ulp above pi wraps.  nb = 2: k = pi exactly, class 1 -> 1 * pi + residual
    ulp = np.float32(np.spacing(np.pi))
    assert np.float64(ulp) == np.spacing(np.pi) and np.pi + np.float64(ulp) == np.nextafter(np.pi, 4.0)
    planted = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, ulp], [0.0, 1.0, 0.0, -ulp]], np.float32)
    got = RR.decode(planted, 2)
    assert got[0] == np.pi
    assert got[1] == np.nextafter(np.pi, 4.0) - 2 * np.pi and got[1] < 0
    assert got[2] == np.pi - np.float64(ulp)
    np.testing.assert_array_equal(got, _host_decode(monkeypatch, planted, 2))
    # nb = 1: the only class, angle = the residual
    one = np.array([[0.7, 3.0], [-1.0, 3.5]], np.float32)
    np.testing.assert_array_equal(RR.decode(one, 1), [np.float64(np.float32(3.0)), np.float64(np.float32(3.5)) - 2 * np.pi])
    np.testing.assert_array_equal(RR.decode(one, 1), _host_decode(monkeypatch, one, 1))


def test_network_transform_agrees_with_get_mat_angle():
    import evaluation
    rng = np.random.default_rng(5)
    cases = []
    for i in range(200):
        scale = (0.1, 3.0, 60.0)[i % 3]
        cases.append((rng.normal(size=3) * scale, rng.uniform(-np.pi, np.pi), rng.normal(size=3) * scale))
    cases.append((rng.normal(size=3), 2.5, np.array([3600.0, -3400.0, 12.0])))     # a centre 5 km out
    cases.append((rng.normal(size=3), -0.3, np.array([-5000.0, 0.0, 0.0])))
    cases.append((np.zeros(3), 0.0, np.zeros(3)))
    cases.append((rng.normal(size=3), np.pi, rng.normal(size=3)))
    worst = 0.0
    for t, a, c in cases:
        t32, c32 = t.astype(np.float32), c.astype(np.float32)
        got = RR.network_transform(t32, a, c32)
        ref = evaluation.get_mat_angle(t32, a, rotation_center=c32)
        bound = 1e-15 * max(1.0, np.linalg.norm(c32.astype(np.float64)) + np.linalg.norm(t32.astype(np.float64)))
        err = np.abs(got - ref).max()
        worst = max(worst, err / bound)
        assert err <= bound, (t, a, c, err, bound)
        np.testing.assert_array_equal(got[:3, :3], ref[:3, :3])
        np.testing.assert_array_equal(got[3], [0.0, 0.0, 0.0, 1.0])
    print("worst error / bound", worst)


# ---- surface -----------------------------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "alignnet_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


CTYPE = {
    "alignnet_handle*": _capi.H, "const float*": _capi.FP, "float*": _capi.FP, "const int64_t*": C.POINTER(C.c_int64), "const int32_t*": C.POINTER(C.c_int32),
    "int32_t*": C.POINTER(C.c_int32), "double*": C.POINTER(C.c_double), "int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double,
    "const alignnet_register_options*": C.POINTER(_capi.RegisterOptions), "const alignnet_register_outputs*": C.POINTER(_capi.RegisterOutputs),
    "const alignnet_outputs*": C.POINTER(_capi.Outputs),
}


def _ctype(decl):
    """'const float* points1' -> the ctypes type of its type part."""
    m = re.match(r"^(.*?)(\w+)$", " ".join(decl.split()))
    return CTYPE[m.group(1).replace(" *", "*").strip()]


def test_header_declares_functions_and_structs_and_capi_binds_them():
    text = _header()
    assert re.search(r"#define\s+ALIGNNET_ABI_VERSION\s+1\b", text) and _capi.ABI_VERSION == 1
    for fn in ("alignnet_register", "alignnet_register_dataset"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % fn, text)
        assert m, fn + " not declared"
        args = [_ctype(a) for a in m.group(1).split(",")]
        res, bound = _capi.SYMBOLS[fn]
        assert res is C.c_int and bound == args, fn
    for name, cls in (("alignnet_register_options", _capi.RegisterOptions), ("alignnet_register_outputs", _capi.RegisterOutputs)):
        m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, text)
        assert m, name + " not declared"
        fields = [(" ".join(f.split())) for f in m.group(1).split(";") if f.strip()]
        assert [re.match(r"^(.*?)(\w+)$", f).group(2) for f in fields] == [f[0] for f in cls._fields_], name
        assert [_ctype(f) for f in fields] == [f[1] for f in cls._fields_], name
    assert C.sizeof(_capi.RegisterOptions) == 32 and _capi.RegisterOptions.radius.offset == 16
    assert C.sizeof(_capi.RegisterOutputs) == 8 * C.sizeof(C.c_void_p)


def test_built_library_exports_register_symbols():
    lib = alignnet3d.load_library()
    for fn in ("alignnet_register", "alignnet_register_dataset"):
        assert hasattr(lib, fn), fn + " is not exported by " + alignnet3d.library_path()
        assert getattr(lib, fn).argtypes == _capi.SYMBOLS[fn][1]
    assert callable(getattr(alignnet3d.Engine, "register")) and callable(getattr(alignnet3d.Engine, "register_rows"))


def test_library_without_the_symbols_raises_engine_error():
    """An earlier build named by ALIGNNET_HIP_LIB loads without the late symbols; asking for them is a clear EngineError, not an AttributeError."""
    eng = object.__new__(alignnet3d.Engine)
    eng._lib, eng._h = types.SimpleNamespace(), None
    for fn in _capi.LATE_SYMBOLS:
        with pytest.raises(alignnet3d.EngineError, match=fn + ".*rebuild"):
            eng._register_fn(fn)
    with pytest.raises(alignnet3d.EngineError):
        eng.register_rows([0], 1)
    with pytest.raises(alignnet3d.EngineError):
        eng.register([np.zeros((3, 3))], [np.zeros((3, 3))])


def test_register_option_parser():
    import train
    ev = lambda **kw: types.SimpleNamespace(evaluation=types.SimpleNamespace(**kw))
    assert train.register_option(ev(), {}) == "host"                       # the default: today's loop
    assert train.register_option(types.SimpleNamespace(), {}) == "host"
    assert train.register_option(ev(register="device"), {}) == "device"
    assert train.register_option(ev(register="host"), {}) == "host"
    assert train.register_option(ev(register="host"), {"ALIGNNET_REGISTER": "device"}) == "device"   # the environment wins
    assert train.register_option(ev(register="device"), {"ALIGNNET_REGISTER": "host"}) == "host"
    assert train.register_option(ev(register="device"), {"ALIGNNET_REGISTER": ""}) == "device"
    for bad_cfg, bad_env in ((ev(register="gpu"), {}), (ev(), {"ALIGNNET_REGISTER": "1"}), (ev(register="device"), {"ALIGNNET_REGISTER": "hosts"})):
        with pytest.raises(ValueError, match="evaluation.register"):
            train.register_option(bad_cfg, bad_env)
