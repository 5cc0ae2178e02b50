"""GPU: the one-call registration (Engine.register / register_rows; csrc/alignnet_register.hip) against the calls it joins.
Everything is like with like on the device's own upstream output, as the global-registration tests do it: the network arrays against
forward_rows of the same draw (bit for bit), the angles against tests/register_ref.decode of those logits (bit for bit), T_net against
register_ref.network_transform (derived bound), the refinement against icp_refine_rows / icp_plane_refine_rows from the call's own T_net (bit for
bit), the loss against eval_loss (bit for bit).  Every test here needs the new entry points."""
import ctypes as C

import numpy as np
import pytest

import alignnet3d
from alignnet3d import _capi
from alignnet3d.engine import OUTPUT_NAMES
from tests import register_ref as RR
from tests.helpers import small_cfg, oracle_params

pytestmark = pytest.mark.gpu
SEED = 20240611
FAR = np.array([3600.0, -3400.0, 10.0])   # 5 km from the origin
# (source points, target points) per example row; rows 0, 1, 6, 7, 8 show ONE object in both clouds (the target is the source moved by a small
# transform and disturbed by a millimetre of noise, so ICP has inliers); row 8 sits 5 km out; 4300 targets is over the `auto` grid threshold (4266)
SIZES = [(300, 300), (1500, 1500), (0, 300), (300, 0), (1, 300), (7, 7), (1500, 4300), (300, 1500), (300, 300), (1500, 300), (300, 1), (7, 300)]
SAME_OBJECT = (0, 1, 6, 7, 8)
LABEL_KEYS = ("translations", "rel_angles", "pc1_centers", "pc2_centers", "pc1_angles", "pc2_angles")


def _dataset():
    rng = np.random.default_rng(7)
    src, dst = [], []
    for i, (n1, n2) in enumerate(SIZES):
        centre = FAR if i == 8 else rng.normal(size=3) * np.array([3.0, 3.0, 0.2])
        obj = lambda n: rng.uniform(-1, 1, (n, 3)) * np.array([2.2, 0.9, 0.7])
        if i in SAME_OBJECT:
            body = obj(max(n1, n2))
            a, t = rng.uniform(-0.2, 0.2), rng.normal(size=3) * np.array([0.15, 0.15, 0.02])
            R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
            s = body[rng.permutation(len(body))[:n1]]
            d = body[rng.permutation(len(body))[:n2]] @ R.T + t + rng.normal(size=(n2, 3)) * 1e-3
        else:
            s, d = obj(n1), obj(n2) + rng.normal(size=3) * 0.3
        src.append((s + centre).astype(np.float32)); dst.append((d + centre).astype(np.float32))
    off = np.zeros((len(SIZES) + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(s) for s in src]); off[1:, 1] = np.cumsum([len(d) for d in dst])
    lab = rng.normal(size=(len(SIZES), 12)).astype(np.float32)
    lab[:, [3, 10, 11]] = rng.uniform(-np.pi, np.pi, (len(SIZES), 3)).astype(np.float32)   # the three angle columns
    return src, dst, off, lab


def _labels(lab, rows):
    L = lab[np.asarray(rows)]
    return dict(translations=L[:, 0:3], rel_angles=L[:, 3:4], pc1_centers=L[:, 4:7], pc2_centers=L[:, 7:10], pc1_angles=L[:, 10:11], pc2_angles=L[:, 11:12])


@pytest.fixture(scope="module", params=[128, 64])
def rig(request, gpu_required):
    cfg = small_cfg(N=request.param, nb=12)
    spec, P32 = oracle_params(cfg)   # BN statistics randomised
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    src, dst, off, lab = _dataset()
    eng.upload_dataset(np.concatenate(src), np.concatenate(dst), off, lab)
    yield dict(eng=eng, src=src, dst=dst, off=off, lab=lab, nb=12, rows=list(range(len(SIZES))), P32=P32, cfg=cfg)
    eng.close()


def _same(a, b, keys, msg=""):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s %s" % (msg, k))


# ---- a. network outputs and angles ------------------------------------------------------------------------------------------------------------------
def test_network_outputs_and_angles(rig):
    eng, rows, nb = rig["eng"], rig["rows"], rig["nb"]
    res = eng.register_rows(rows, SEED, want_net=True)
    fw = eng.forward_rows(rows, SEED)
    _same(res, fw, OUTPUT_NAMES, "register_rows vs forward_rows")
    a1, a2, ar = (RR.decode(fw[k], nb) for k in ("pred_pc1angle_logits", "pred_pc2angle_logits", "pred_remaining_angle_logits"))
    want = np.stack([a1, a2, ar, RR.pred_angle(a1, a2, ar)], 1)
    assert res["angles"].dtype == np.float64
    np.testing.assert_array_equal(res["angles"], want)
    assert res["loss"] is None and "fitness" not in res
    np.testing.assert_array_equal(res["transforms"], res["network_transforms"])   # no refinement: the final estimate is T_net
    assert (want[:, :3] > 0).any() and (want[:, :3] < 0).any()
    # without want_net the same transforms, and no network arrays
    lean = eng.register_rows(rows, SEED)
    _same(lean, res, ("transforms", "network_transforms", "angles"))
    assert not set(OUTPUT_NAMES) & set(lean)
    # another seed is another draw
    assert not np.array_equal(eng.register_rows(rows, SEED + 1)["angles"], res["angles"])


def test_exact_tie_of_the_top_two_classes_first_wins(gpu_required):
    """The class logits of both towers are made exactly equal at classes 4 and 9 (and lower elsewhere) through the last layer of the stage-2 head:
    zero weights into the class columns, the planted values as biases (0 * x + b = b exactly).  np.argmax and the kernel must both take class 4."""
    nb = 12
    cfg = small_cfg(N=64, nb=nb)
    spec, P32 = oracle_params(cfg)
    P = dict(P32)
    W, b = P["siamese/transformer2/mlp/fc3/weights"].copy(), P["siamese/transformer2/mlp/fc3/biases"].copy()
    W[:, 3:3 + nb] = 0.0
    b[3:3 + nb] = np.linspace(-1.0, 0.5, nb).astype(np.float32)
    b[3 + 4] = b[3 + 9] = np.float32(1.25)
    P["siamese/transformer2/mlp/fc3/weights"], P["siamese/transformer2/mlp/fc3/biases"] = W, b
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P)
    src, dst, off, lab = _dataset()
    eng.upload_dataset(np.concatenate(src), np.concatenate(dst), off, lab)
    rows = [0, 5, 8, 2]
    res = eng.register_rows(rows, SEED, want_net=True)
    for k in ("pred_pc1angle_logits", "pred_pc2angle_logits"):
        cls = res[k][:, :nb]
        assert np.all(cls[:, 4] == cls[:, 9]) and np.all(cls.max(1) == cls[:, 4]), "the tie did not reach the logits"
        assert np.all(np.argmax(cls, 1) == 4)
    k = 2 * np.pi / nb
    np.testing.assert_array_equal(res["angles"][:, 0], 4 * k + res["pred_pc1angle_logits"][:, nb + 4].astype(np.float64))
    np.testing.assert_array_equal(res["angles"][:, 1], RR.decode(res["pred_pc2angle_logits"], nb))
    np.testing.assert_array_equal(res["angles"][:, 2], RR.decode(res["pred_remaining_angle_logits"], nb))
    eng.close()


# ---- b. network transform -----------------------------------------------------------------------------------------------------------------------------
def test_network_transform(rig):
    """Bound 1e-13 max(1, |c| + |t|), derived: the device's fp64 sin / cos are within a few ulps (2.2e-16 each) of NumPy's and multiply the lever
    arm |c|, the sums of three terms of magnitude <= |c| + |t| round a few times more: a few 1e-16 (|c| + |t|) in all, under the bound by two orders."""
    eng, rows = rig["eng"], rig["rows"]
    res = eng.register_rows(rows, SEED, want_net=True)
    worst = 0.0
    for b in rows:
        t, c = res["pred_translations"][b], res["pred_s2_pc1centers"][b]
        want = RR.network_transform(t, res["angles"][b, 3], c)
        bound = 1e-13 * max(1.0, np.linalg.norm(c.astype(np.float64)) + np.linalg.norm(t.astype(np.float64)))
        err = np.abs(res["network_transforms"][b] - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
        np.testing.assert_array_equal(res["network_transforms"][b][3], [0, 0, 0, 1])
        np.testing.assert_array_equal(res["network_transforms"][b][2, :3], [0, 0, 1])
    print("T_net: worst error / bound %.3g" % worst)
    assert np.linalg.norm(res["pred_s2_pc1centers"][8]) > 4000.0   # the far pair's rotation centre is far: the lever arm is exercised


# ---- c. refinement ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", ["point", "plane"])
@pytest.mark.parametrize("constrained", [True, False])
def test_refinement_equals_icp_from_own_network_transform(rig, refine, constrained):
    eng, rows = rig["eng"], rig["rows"]
    inliers = 0
    try:
        for search in (0, 1, 2):
            eng.set_option("icp_search", search)
            for its in (0, 1, 30):
                for radius in ((0.1, 1.0) if its == 30 else (1.0,)):
                    kw = dict(radius=radius, its=its, constrained=constrained)
                    if refine == "plane":
                        kw["normal_radius"] = 0.3
                    res = eng.register_rows(rows, SEED, refine=refine, **kw)
                    fn = eng.icp_refine_rows if refine == "point" else eng.icp_plane_refine_rows
                    ref = fn(rows, res["network_transforms"], **kw)
                    _same(res, ref, ("transforms", "fitness", "rmse", "iterations"), "%s search %d its %d radius %g" % (refine, search, its, radius))
                    assert res["iterations"].dtype == np.int32 and res["iterations"].max() <= its
                    if its == 30 and radius == 1.0:
                        inliers = max(inliers, int((res["fitness"] > 0.2).sum()))
                        assert (res["iterations"] > 1).any()
                        assert not np.array_equal(res["transforms"], res["network_transforms"])
                    for b in (2, 3):   # an empty cloud: ICP leaves the pair at T_net
                        np.testing.assert_array_equal(res["transforms"][b], res["network_transforms"][b])
    finally:
        eng.set_option("icp_search", 0)
    print("%s constrained=%s: pairs with fitness > 0.2 at radius 1.0: %d" % (refine, constrained, inliers))
    assert inliers >= 3, "the refinement had nothing to refine: the comparison above would be vacuous"


# ---- d. host clouds -----------------------------------------------------------------------------------------------------------------------------------
def test_host_clouds(rig):
    eng, src, dst = rig["eng"], rig["src"], rig["dst"]
    rows = [6, 0, 2, 3, 8, 4, 11]
    S, D = [src[r] for r in rows], [dst[r] for r in rows]
    for refine in (None, "point", "plane"):
        host = eng.register(S, D, seed=SEED, streams=rows, refine=refine, want_net=True)
        dev = eng.register_rows(rows, SEED, refine=refine, want_net=True)
        _same(host, dev, OUTPUT_NAMES + ("angles", "network_transforms"), "host vs rows, refine %s" % refine)
        if refine:
            fn = eng.icp_refine if refine == "point" else eng.icp_plane_refine
            ref = fn(S, D, host["network_transforms"])
            _same(host, ref, ("transforms", "fitness", "rmse", "iterations"), "host refine %s" % refine)
    # streams=None is the pair index
    none = eng.register(S, D, seed=SEED, want_net=True)
    ar = eng.register(S, D, seed=SEED, streams=np.arange(len(rows)), want_net=True)
    _same(none, ar, OUTPUT_NAMES + ("angles", "network_transforms", "transforms"))
    assert not np.array_equal(none["angles"], eng.register(S, D, seed=SEED, streams=rows)["angles"])
    # smaller clouds after larger ones reuse the workspace
    one = eng.register(S[1:2], D[1:2], seed=SEED, streams=rows[1:2], refine="point")
    np.testing.assert_array_equal(one["transforms"][0], eng.register_rows(rows[1:2], SEED, refine="point")["transforms"][0])


# ---- e. batch independence ----------------------------------------------------------------------------------------------------------------------------
def test_batch_independence_and_order(rig):
    """The point tile of the eval backbone is fixed (by default it is chosen from the batch size, and another tile is another summation order: the
    forward tests fix it the same way)."""
    eng, rows = rig["eng"], rig["rows"]
    eng.set_option("infer_tile_points", 64)
    try:
        keys = OUTPUT_NAMES + ("angles", "network_transforms", "transforms", "fitness", "rmse", "iterations")
        kw = dict(refine="point", radius=1.0, want_net=True)
        full = eng.register_rows(rows, SEED, **kw)
        five = {}
        for lo in range(0, 12, 5):
            part = rows[lo:lo + 5] if lo + 5 <= 12 else rows[7:12]
            r5 = eng.register_rows(part, SEED, **kw)
            for j, b in enumerate(part):
                five[b] = {k: r5[k][j] for k in keys}
        for b in rows:
            alone = eng.register_rows([b], SEED, **kw)
            for k in keys:
                np.testing.assert_array_equal(alone[k][0], full[k][b], err_msg="pair %d alone vs in 12: %s" % (b, k))
                np.testing.assert_array_equal(alone[k][0], five[b][k], err_msg="pair %d alone vs in 5: %s" % (b, k))
        perm = np.random.default_rng(3).permutation(12)
        shuffled = eng.register_rows(perm, SEED, **kw)
        for k in keys:
            np.testing.assert_array_equal(shuffled[k], full[k][perm], err_msg="permuted rows: " + k)
    finally:
        eng.set_option("infer_tile_points", 0)


# ---- f. loss ------------------------------------------------------------------------------------------------------------------------------------------
def test_loss_equals_eval_loss(rig):
    eng, lab = rig["eng"], rig["lab"]
    for rows in (rig["rows"], [0, 1, 5, 7, 9]):
        for refine in (None, "point"):
            res = eng.register_rows(rows, SEED, refine=refine, want_loss=True)
            eng.forward_rows(rows, SEED)
            loss, summ = eng.eval_loss(_labels(lab, rows), len(rows))
            assert res["loss"][0] == loss and np.isfinite(loss)
            assert res["loss"][1] == summ


# ---- g. errors ----------------------------------------------------------------------------------------------------------------------------------------
def _raw(eng, opt, out, rows=(0, 1)):
    r = np.asarray(rows, np.int32)
    return eng._lib.alignnet_register_dataset(eng._h, r.ctypes.data_as(C.POINTER(C.c_int32)), r.size, 1, C.byref(opt) if opt is not None else None,
                                              C.byref(out) if out is not None else None)


def test_errors_leave_the_engine_as_it_was(rig):
    eng, src, dst, rows = rig["eng"], rig["src"], rig["dst"], rig["rows"]
    E = alignnet3d.EngineError
    keys = ("transforms", "network_transforms", "angles", "fitness", "rmse", "iterations")
    before = eng.register_rows(rows, SEED, refine="point", radius=1.0)
    icp_before = eng.icp_refine_rows(rows, before["network_transforms"], radius=1.0)
    fw_before = eng.forward_rows(rows, SEED)
    S, D = [src[r] for r in (0, 5)], [dst[r] for r in (0, 5)]
    host_before = eng.register(S, D, seed=SEED, refine="plane")

    def check_unchanged():
        _same(eng.register_rows(rows, SEED, refine="point", radius=1.0), before, keys, "after an error")
        _same(eng.register(S, D, seed=SEED, refine="plane"), host_before, keys, "after an error (host)")

    # B < 1, row out of range, bad option values
    for bad in (lambda: eng.register_rows([], SEED), lambda: eng.register([], [], seed=SEED),
                lambda: eng.register_rows([0, len(SIZES)], SEED), lambda: eng.register_rows([-1], SEED),
                lambda: eng.register_rows(rows, SEED, refine="point", radius=0.0), lambda: eng.register_rows(rows, SEED, refine="point", radius=float("nan")),
                lambda: eng.register_rows(rows, SEED, refine="point", its=-1), lambda: eng.register_rows(rows, SEED, refine="plane", normal_radius=0.0),
                lambda: eng.register(S, D, seed=SEED, refine="plane", normal_radius=-1.0)):
        with pytest.raises(E):
            bad()
    with pytest.raises(ValueError):
        eng.register_rows(rows, SEED, refine="p2p")
    with pytest.raises(ValueError):
        eng.register(S, D[:1], seed=SEED)
    check_unchanged()
    # through the C ABI: null arguments, its without refinement, results of a refinement that does not run, unknown flags / refine, the loss on host clouds
    T = np.empty((2, 16)); fit = np.empty(2)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    good_out = _capi.RegisterOutputs(); good_out.transforms = dp(T)
    assert _raw(eng, _capi.RegisterOptions(0, 0, 0, 0.1, 0.3), good_out) == 0
    assert _raw(eng, None, good_out) != 0 and _raw(eng, _capi.RegisterOptions(0, 0, 0, 0.1, 0.3), None) != 0
    assert _raw(eng, _capi.RegisterOptions(0, 0, 0, 0.1, 0.3), _capi.RegisterOutputs()) != 0              # transforms is null
    assert b"transforms" in eng._lib.alignnet_last_error(eng._h)
    assert _raw(eng, _capi.RegisterOptions(0, 5, 0, 0.1, 0.3), good_out) != 0                             # its without refinement
    fit_out = _capi.RegisterOutputs(); fit_out.transforms = dp(T); fit_out.fitness = dp(fit)
    assert _raw(eng, _capi.RegisterOptions(0, 0, 0, 0.1, 0.3), fit_out) != 0                              # fitness without refinement
    assert _raw(eng, _capi.RegisterOptions(1, 5, 0, 0.1, 0.3), fit_out) == 0
    for opt in (_capi.RegisterOptions(3, 5, 0, 0.1, 0.3), _capi.RegisterOptions(-1, 0, 0, 0.1, 0.3), _capi.RegisterOptions(1, 5, 2, 0.1, 0.3),
                _capi.RegisterOptions(1, 5, 3, 0.1, 0.3), _capi.RegisterOptions(2, 5, 0, 0.1, float("nan"))):
        assert _raw(eng, opt, good_out) != 0
    assert eng._lib.alignnet_register_dataset(eng._h, None, 2, 1, C.byref(_capi.RegisterOptions(0, 0, 0, 0.1, 0.3)), C.byref(good_out)) != 0   # null rows
    off = np.array([[0, 0], [3, 3], [2, 6]], np.int64)   # decreasing offsets
    pts = np.zeros((8, 3), np.float32)
    host = lambda o, p1=pts, p2=pts, out=good_out: eng._lib.alignnet_register(
        eng._h, p1.ctypes.data_as(_capi.FP) if p1 is not None else None, p2.ctypes.data_as(_capi.FP) if p2 is not None else None,
        o.ctypes.data_as(C.POINTER(C.c_int64)) if o is not None else None, 2, 1, None, C.byref(_capi.RegisterOptions(0, 0, 0, 0.1, 0.3)), C.byref(out))
    assert host(off) != 0 and b"non-decreasing" in eng._lib.alignnet_last_error(eng._h)
    assert host(None) != 0
    assert host(np.array([[-1, 0], [3, 3], [4, 6]], np.int64)) != 0
    ok_off = np.array([[0, 0], [3, 3], [4, 6]], np.int64)
    assert host(ok_off, None) != 0 and host(ok_off, pts, None) != 0                                      # null blobs with points in them
    loss_out = _capi.RegisterOutputs(); loss_out.transforms = dp(T); loss17 = np.empty(17, np.float32); loss_out.loss = loss17.ctypes.data_as(_capi.FP)
    assert host(ok_off, out=loss_out) != 0                                                               # the loss needs the dataset's labels
    assert host(ok_off) == 0
    check_unchanged()
    # the existing calls on this data are what they were
    _same(eng.icp_refine_rows(rows, before["network_transforms"], radius=1.0), icp_before, ("transforms", "fitness", "rmse", "iterations"))
    _same(eng.forward_rows(rows, SEED), fw_before, OUTPUT_NAMES)


def test_no_dataset_is_an_error_and_host_clouds_need_none(gpu_required):
    cfg = small_cfg(N=64, nb=12)
    spec, P32 = oracle_params(cfg)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    with pytest.raises(alignnet3d.EngineError, match="no dataset"):
        eng.register_rows([0], SEED)
    src, dst, off, lab = _dataset()
    res = eng.register(src[:2], dst[:2], seed=SEED, refine="point", radius=1.0)
    assert np.all(np.isfinite(res["transforms"]))
    eng.upload_dataset(np.concatenate(src), np.concatenate(dst), off, lab)
    np.testing.assert_array_equal(eng.register_rows([0, 1], SEED, refine="point", radius=1.0)["transforms"], res["transforms"])
    eng.close()
