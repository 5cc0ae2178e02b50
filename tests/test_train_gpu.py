"""GPU parity of the training path through the C ABI: train-mode forward (batch statistics, EMA),
loss, every parameter gradient and the optimiser step vs the torch-autograd oracle (fp64) on the same
fp32-representable parameters, inputs and dropout uniforms."""
import numpy as np
import pytest
import torch

import alignnet3d
from oracle import alignnet_ref as R
from oracle import alignnet_torch as T
from tests.helpers import small_cfg, oracle_params

pytestmark = pytest.mark.gpu
LABELS = ("translations", "rel_angles", "pc1_centers", "pc2_centers", "pc1_angles", "pc2_angles")


def _oracle(cfg, P32, d, du, decay, bf16_lift=False, dt=np.float64, checkpoint=False, pinned=None, report=None):
    """pinned: the engine's decisions (Engine.debug_train_decisions) -- the oracle gathers at them instead of deciding itself
    (oracle/alignnet_torch.py); report: a list that receives the oracle's check of every pinned decision."""
    spec = R.NetSpec.from_cfg(cfg)
    tp = T.to_torch({k: v.astype(dt) for k, v in P32.items()}, dtype=torch.float64 if dt == np.float64 else torch.float32, requires_grad=True)
    tm = T.TorchTp8(spec, tp, bf16_lift=bf16_lift, checkpoint=checkpoint, pinned=pinned)
    if report is not None:
        report.append(tm.pin_report)   # (filled while forward / backward run)
    td = {k: torch.tensor(v.astype(dt)) for k, v in d.items()}
    tu = {k: torch.tensor(v.astype(dt)) for k, v in du.items()}
    ep = tm.forward(td["pcs1"], td["pcs2"], True, decay, tu)
    loss = tm.loss(ep, *[td[k] for k in LABELS])
    loss.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in tp.items() if v.requires_grad}
    return ({k: v.detach().numpy() for k, v in ep.items()}, float(loss.detach()), grads,
            {k: v.numpy() for k, v in tm.ema_updates.items()})


STD = dict(s1=(64, 128, 96), s2=(64, 128, 128), emb=(64, 128, 160))   # first two widths of every shipped config: the
# engine runs kernel instantiations with these widths compiled in (alignnet_train.hip: std_w)


def _setup(N, B, nb=12, seed=5, std=False):
    w = STD if std else dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(32, 64, 160))
    cfg = small_cfg(N=N, nb=nb, fc=(64, 32), **w)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=seed)
    # BN-preceding biases have an identically-zero gradient; keep them non-zero to test that path
    d = R.synth_pairs(B, N, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed)
    du = {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
    return cfg, spec, P32, d, du


def _rel_err(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.mark.parametrize("N,B", [(128, 6), (200, 4)])
def test_train_forward_loss_ema(gpu_required, N, B):
    cfg, spec, P32, d, du = _setup(N, B)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    st = eng.state()
    ep_ref, loss_ref, _, ema_ref = _oracle(cfg, P32, d, du, st["bn_decay"])
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    for k in ep_ref:
        np.testing.assert_allclose(res[k], ep_ref[k], rtol=2e-4, atol=2e-4, err_msg=k)
    assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    worst = 0.0
    for k, v in ema_ref.items():
        got = eng.get_variable(k)
        np.testing.assert_allclose(got, v, rtol=1e-4, atol=1e-5, err_msg=k)
        worst = max(worst, float(np.abs(got - v).max()))
    print("loss", res["loss"], loss_ref, "worst EMA abs err", worst)
    eng.close()


@pytest.mark.parametrize("N,B,tol,std", [(256, 16, 5e-4, False), (128, 6, 1e-2, False), (192, 12, 1e-3, True)])
def test_gradients_match_autograd(gpu_required, N, B, tol, std):
    """Every trainable tensor.  Tolerance: relative to the tensor's largest reference entry, plus an absolute
    floor of 1e-5 x the largest gradient entry of the whole model for tensors whose exact gradient is zero
    (e.g. the beta of a BN whose output feeds another BN through a linear map, biases in front of a BN).
    B = 6 is a conditioning stress case (6-row batch statistics amplify fp32 forward differences)."""
    cfg, spec, P32, d, du = _setup(N, B, std=std)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    _, _, grads, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=eng.debug_train_decisions(B, relu=True))   # (pinned to this step's decisions and relu signs)
    gscale = max(float(np.abs(v).max()) for v in grads.values())
    report, bad = {}, {}
    bn_bias = set()
    for L in R.layer_table(spec):
        if L.bn:
            bn_bias.add((f"siamese/{L.name}" if L.siamese else L.name) + "/biases")
    for name in R.trainable_names(spec):
        g = eng.get_gradient(name).astype(np.float64)
        ref = grads[name].reshape(g.shape)
        if name in bn_bias:
            # bias in front of a BatchNorm: the exact gradient is 0 (autograd returns rounding noise, TF too)
            assert np.abs(g).max() == 0.0 and np.abs(ref).max() < 1e-9 * gscale, name
            continue
        err = float(np.abs(g - ref).max())
        report[name] = err / (float(np.abs(ref).max()) + 1e-30)
        if err > tol * float(np.abs(ref).max()) + 1e-5 * gscale:
            bad[name] = (err, float(np.abs(ref).max()))
    real = {k: v for k, v in report.items() if np.abs(grads[k]).max() > 1e-6 * gscale}
    print("worst relative gradient errors:", sorted(real.items(), key=lambda kv: -kv[1])[:5])
    assert not bad, bad
    eng.close()


def test_deep_heads_flush_their_jobs_in_chunks(gpu_required):
    """Six FC layers per head: 3 x 6 deferred dW products + the six of the conv layers = 24 jobs, more than one job table of the deferred
    launches holds (kGemmJobs = 18; round 3 failed such a step with "job table overflow" after the backward had been queued -- ADVICE round 3).
    flush_deferred chunks its tables; every gradient against autograd, and the same step with deferral off (ab_no_defer)."""
    N, B = 128, 16
    cfg = small_cfg(N=N, nb=12, fc=(64, 48, 40, 32, 24), s1=(32, 64, 96), s2=(32, 64, 128), emb=(32, 64, 160))
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=5)
    d = R.synth_pairs(B, N, seed=5, dtype=np.float32)
    rng = np.random.default_rng(5)
    du = {k: rng.uniform(size=(B, 24)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}   # (dropout sits behind the last hidden layer)
    ul = [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")]
    got = []
    for nodefer in (0, 1):
        eng = alignnet3d.Engine(cfg)
        eng.set_variables(P32)
        eng.set_option("ab_no_defer", nodefer)
        res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, ul)
        got.append({n: eng.get_gradient(n).astype(np.float64) for n in R.trainable_names(spec)})
        if not nodefer:
            # the oracle PINNED to this step's decisions and relu signs (a unit of one of the 36 sixteen-row BatchNorms within a rounding of zero is
            # "on" in one evaluation and "off" in the other, and a free comparison then reads 1e-2: measured when the head backward's mask
            # expression changed in round 6)
            _, loss_ref, grads, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=eng.debug_train_decisions(B, relu=True))
        assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref))
        eng.close()
    # six BatchNorm'd layers on 16-row statistics are badly conditioned (gradient entries of several hundred, the fp32 forward's rounding amplified
    # layer by layer): against autograd the whole gradient is compared; the sharp check is deferred == in place
    names = list(got[0])
    ga = np.concatenate([got[0][n].ravel() for n in names]); gr = np.concatenate([grads[n].ravel() for n in names])
    rl2 = float(np.linalg.norm(ga - gr) / np.linalg.norm(gr)); cos = float(ga @ gr / (np.linalg.norm(ga) * np.linalg.norm(gr)))
    print("deep heads: whole gradient vs autograd: relative L2 %.2e, cosine %.6f" % (rl2, cos))
    assert rl2 <= 2e-3 and cos >= 0.99999, (rl2, cos)   # measured 1.0e-4
    gscale = float(np.abs(ga).max())
    for n in names:
        np.testing.assert_allclose(got[1][n], got[0][n], rtol=1e-4, atol=1e-5 * gscale, err_msg=n)   # deferred == in place, up to summation order


def test_adam_step_and_state(gpu_required):
    cfg, spec, P32, d, du = _setup(128, 6)
    cfg["data"]["ntrain"] = 600
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    _, _, grads, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"])
    lr = eng.state()["learning_rate"]
    assert abs(lr - 0.005) < 1e-9
    res = eng.train_step(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    assert res["step"] == 1 and eng.state()["step"] == 1
    for name in ("siamese/embedding/conv3/weights", "fc1/weights", "siamese_1/transformer2/embedding/conv2/bn/gamma"):
        w0 = P32[name].astype(np.float64)
        g = grads[name]
        w1, _, _ = R.adam_step(w0, g, np.zeros_like(g), np.zeros_like(g), 1, lr)
        got = eng.get_variable(name)
        # first Adam step ~ lr*sign(g): compare where the gradient is not tiny
        mask = np.abs(g) > 1e-3 * np.abs(g).max()
        np.testing.assert_allclose(got.reshape(w0.shape)[mask], w1[mask], rtol=0, atol=2e-4 * lr + 1e-7, err_msg=name)
    eng.close()


def test_save_load_roundtrip(gpu_required, tmp_path):
    cfg, spec, P32, d, du = _setup(128, 4)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    eng.train_step(d["pcs1"], d["pcs2"], d)
    path = tmp_path / "model-0.aln3"
    eng.save(path)
    ref = eng.forward(d["pcs1"], d["pcs2"])
    eng2 = alignnet3d.Engine(cfg)
    eng2.load(path)
    assert eng2.state()["step"] == 1
    out = eng2.forward(d["pcs1"], d["pcs2"])
    for k in ref:
        np.testing.assert_array_equal(ref[k], out[k])
    eng3 = alignnet3d.Engine(cfg)
    eng3.load(path, skip_step=True)   # pre-training restore excludes `batch` (train.py:278-281)
    assert eng3.state()["step"] == 0
    with pytest.raises(alignnet3d.EngineError):
        eng3.load(tmp_path / "missing.aln3")
    for e in (eng, eng2, eng3):
        e.close()


def test_eval_loss_matches_oracle(gpu_required):
    cfg, spec, P32, d, _ = _setup(128, 6)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    eng.forward(d["pcs1"], d["pcs2"])
    loss, summ = eng.eval_loss(d, 6)
    P64 = {k: v.astype(np.float64) for k, v in P32.items()}
    ep, _, _ = R.get_model(P64, spec, d["pcs1"].astype(np.float64), d["pcs2"].astype(np.float64))
    lref, sref = R.get_loss(spec, ep, *[d[k].astype(np.float64) for k in LABELS])
    assert abs(loss - lref) <= 1e-4 * max(1.0, abs(lref)), (loss, lref)
    for k, v in sref.items():
        assert abs(summ[k] - v) <= 2e-4 * max(1.0, abs(v)), (k, summ[k], v)
    eng.close()


@pytest.mark.parametrize("N,B,std", [(256, 64, False), (200, 48, False), (192, 48, True)])
def test_bf16_lift_matches_rounded_oracle(gpu_required, N, B, std):
    """BASELINE.json configs[2] (bf16 training): option "train_matmul_bf16" runs the MFMA convs of every backbone (hidden
    layer and lift, forward and the backward's recompute) on bf16 MFMA (operands rounded to nearest even, fp32
    accumulation); the backward otherwise treats the rounding as identity (straight-through).  The oracle
    models exactly that (TorchTp8(bf16_lift=True): same rounding, exact accumulation).  What remains between the two is
    rounding-boundary noise: an fp32-vs-fp64 difference in h2 moves some entries to the neighbouring bf16 value (one
    ulp = 0.4 % of one product), and a moved entry on an arg-max row shifts one pooled feature of one sample.
    Tolerances (written here):
      * batch statistics of the bf16 lift (read back through the EMA shadows, averages over B*N rows): 1e-4 relative to
        the largest entry, and >= 10x closer to the rounded oracle than the fp32 step is;
      * stage-1 centres (identical inputs): median per-sample error <= 1e-3, max <= 2e-2; later predictions: max <= 1e-1
        (samples whose argmax yaw decode differs from the oracle's are counted and bounded; the stage-3 outputs, which are
        batch-normalised together, are only compared when there is none);
        every prediction >= 5x closer to the rounded oracle than the fp32 step's;
      * loss within 5e-3 (5e-2 with decode flips); whole gradient within cosine 0.97 (0.85 with flips) of the oracle's (a moved arg-max row re-routes that
        channel's gradient to another point) and >= 3x closer (1 - cos) than the fp32 step's gradient.
    Against the *fp32* step the bf16 step differs by ~1 % in the stage features and flips a few argmax yaw decodes per
    batch (tools/bf16_check.py), which is why the comparison is against the rounded oracle."""
    cfg, spec, P32, d, du = _setup(N, B, std=std)
    bf16_check(cfg, spec, P32, d, du, B, expect_kernel=3 if std else 2)


def bf16_check(cfg, spec, P32, d, du, B, expect_kernel, checkpoint=False):
    """Body of test_bf16_lift_matches_rounded_oracle (also run at BASELINE.json's full size by tests/test_fullsize_gpu.py)."""
    us = [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")]
    stats = ["siamese/transformer1/embedding/conv3/bn/moving_mean", "siamese_1/transformer1/embedding/conv3/bn/moving_var"]
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    assert eng.get_option("train_matmul_bf16") == 0
    res32 = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
    ema32 = {k: eng.get_variable(k) for k in stats}
    g32 = np.concatenate([eng.get_gradient(n).astype(np.float64).ravel() for n in R.trainable_names(spec)])
    eng.set_variables(P32)
    eng.set_option("train_matmul_bf16", 1)
    assert eng.get_option("train_matmul_bf16") == 1
    ep_ref, loss_ref, grads, ema_ref = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], bf16_lift=True, checkpoint=checkpoint)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
    assert res["loss"] != res32["loss"], "bf16 option had no effect"
    assert eng.get_option("last_train_kernel") == expect_kernel   # bit 0: widths (64, 128) compiled in, bit 1: bf16 operands
    for k in stats:
        got, ref = eng.get_variable(k), ema_ref[k]
        e16, e32 = float(np.abs(got - ref).max()), float(np.abs(ema32[k] - ref).max())
        print(k, "err vs rounded oracle %.2e (fp32 step: %.2e), scale %.2e" % (e16, e32, np.abs(ref).max()))
        assert e16 <= 1e-4 * np.abs(ref).max() and e16 < 0.1 * e32, (k, e16, e32)
    nb = spec.num_bins
    # the yaw decode between the stages is an argmax (tp8.py:294-301): a sample whose decoded class differs between the engine
    # and the rounded oracle feeds a different frame to stage 3 -- such samples are counted and left out of the stage-3 checks
    flipped = np.zeros(B, bool)
    for k in ("pred_pc1angle_logits", "pred_pc2angle_logits"):
        flipped |= np.argmax(res[k][:, :nb], 1) != np.argmax(ep_ref[k][:, :nb], 1)
    print("decode flips vs the rounded oracle:", int(flipped.sum()), "of", B)
    assert flipped.sum() <= max(2, B // 16)
    for k in ep_ref:
        per = np.abs(res[k] - ep_ref[k]).reshape(B, -1).max(1)
        err32 = float(np.abs(res32[k] - ep_ref[k]).max())
        if k in ("pred_translations", "pred_remaining_angle_logits") and flipped.any():
            continue   # the pair head normalises over the batch: a flipped sample moves every row of its output
        print(k, "median %.2e max %.2e (fp32 step max %.2e)" % (np.median(per), per.max(), err32))
        if "s1_" in k:
            assert np.median(per) <= 1e-3 and per.max() <= 2e-2, (k, per.max())
        assert per.max() <= 1e-1 and per.max() < 0.2 * err32, (k, per.max(), err32)
    clean = not flipped.any()
    assert abs(res["loss"] - loss_ref) <= (5e-3 if clean else 5e-2) * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    g16 = {n: eng.get_gradient(n).astype(np.float64).ravel() for n in R.trainable_names(spec)}
    a, b = np.concatenate(list(g16.values())), np.concatenate([grads[n].ravel() for n in g16])
    cos_all = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
    cos32 = float(g32 @ b / (np.linalg.norm(g32) * np.linalg.norm(b)))
    print("loss", res["loss"], loss_ref, "fp32 step", res32["loss"], "gradient cosine", cos_all, "fp32 step's", cos32)
    assert cos_all > (0.97 if clean else 0.85) and (1 - cos_all) < (0.3 if clean else 0.7) * (1 - cos32)
    with pytest.raises(RuntimeError):
        eng.set_option("no_such_option", 1)
    eng.close()


def _setup_dgcnn(N, B, seed=7, std=False):
    w = STD if std else dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(64, 128, 160))
    cfg = small_cfg(N=N, fc=(64, 32), backbone="dgcnn", **w)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=seed)
    d = R.synth_pairs(B, N, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed)
    du = {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
    return cfg, spec, P32, d, du


@pytest.mark.parametrize("N,B", [(128, 6), (96, 4)])
def test_dgcnn_train_forward_loss_ema(gpu_required, N, B):
    """DGCNN branch (tp8.py:30-46) in training mode: batch statistics over the B*N*k edge rows, EMA, loss."""
    cfg, spec, P32, d, du = _setup_dgcnn(N, B)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    st = eng.state()
    ep_ref, loss_ref, _, ema_ref = _oracle(cfg, P32, d, du, st["bn_decay"])
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    for k in ep_ref:
        np.testing.assert_allclose(res[k], ep_ref[k], rtol=2e-4, atol=2e-4, err_msg=k)
    assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    worst = 0.0
    for k, v in ema_ref.items():
        got = eng.get_variable(k)
        np.testing.assert_allclose(got, v, rtol=1e-4, atol=1e-5, err_msg=k)
        worst = max(worst, float(np.abs(got - v).max()))
    print("dgcnn loss", res["loss"], loss_ref, "worst EMA abs err", worst)
    eng.close()


@pytest.mark.parametrize("N,B,tol,std", [(128, 8, 2e-3, False), (96, 4, 1e-2, False), (128, 16, 3e-3, True)])
def test_dgcnn_gradients_match_autograd(gpu_required, N, B, tol, std):
    """Every trainable tensor of the DGCNN model against torch autograd (fp64), same criterion as the PointNet test.
    The model takes 20x more max decisions than PointNet (k-max per point and channel), and in fp32 a near-tie routes a
    gradient to another edge row: the SAME oracle evaluated in fp32 is 1e-2..3e-2 away from its fp64 evaluation on some
    tensors (tools/dgcnn_grad_dist.py).  The widest case (std: the 64/128 widths of the shipped configs, kernel
    instantiations with the widths compiled in) therefore bounds the HIP error by twice the fp32 oracle's own error."""
    cfg, spec, P32, d, du = _setup_dgcnn(N, B, std=std)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    _, _, grads, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=eng.debug_train_decisions(B, relu=True))   # (pinned to this step's decisions and relu signs)
    rel32 = 0.0
    if std:
        _, _, g32, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], dt=np.float32, pinned=eng.debug_train_decisions(B, relu=True))
        gs = max(float(np.abs(v).max()) for v in grads.values())
        rel32 = max(float(np.abs(g32[k].astype(np.float64) - grads[k]).max()) / (float(np.abs(grads[k]).max()) + 1e-5 * gs) for k in grads)
        tol = max(tol, 2.0 * rel32)
    gscale = max(float(np.abs(v).max()) for v in grads.values())
    report, bad = {}, {}
    bn_bias = set()
    for L in R.layer_table(spec):
        if L.bn:
            bn_bias.add((f"siamese/{L.name}" if L.siamese else L.name) + "/biases")
    for name in R.trainable_names(spec):
        g = eng.get_gradient(name).astype(np.float64)
        ref = grads[name].reshape(g.shape)
        if name in bn_bias:
            assert np.abs(g).max() == 0.0 and np.abs(ref).max() < 1e-9 * gscale, name
            continue
        err = float(np.abs(g - ref).max())
        report[name] = err / (float(np.abs(ref).max()) + 1e-30)
        if err > tol * float(np.abs(ref).max()) + 1e-5 * gscale:
            bad[name] = (err, float(np.abs(ref).max()))
    real = {k: v for k, v in report.items() if np.abs(grads[k]).max() > 1e-6 * gscale}
    print("dgcnn worst relative gradient errors:", sorted(real.items(), key=lambda kv: -kv[1])[:4], "fp32 oracle vs fp64 oracle:", rel32)
    assert not bad, bad
    eng.close()


@pytest.mark.parametrize("N,B,std", [(128, 8, False), (96, 6, True)])
def test_dgcnn_bf16_convs_match_rounded_oracle(gpu_required, N, B, std):
    """"train_matmul_bf16" with the dgcnn backbone: the edge conv behind the K = 6 lift (z2 = h1 W2 over the B*N*k edge rows, with
    Gram(h1): dg_train_fwd<C1, true>) and the point conv (z3 = p W3, with Gram(p): train_fwd_phase23<3, true, true>) run on bf16
    MFMA with their operands rounded to nearest even; the statistics of z2 follow from the Gram of the ROUNDED h1 with the rounded
    W2; the whole backward stays fp32.  The oracle models the forward exactly (TorchTp8(bf16_lift=True) rounds the operands of the
    edge convs i >= 1 and of the point conv) with a straight-through backward that uses the rounded operands, which the engine's
    fp32 backward does not (it recomputes h1 unrounded and uses the unrounded weights: one bf16 ulp = 0.4 % per operand).
    Tolerances (written here, those of the PointNet bf16 test):
      * batch statistics of the rounded convs (EMA shadows of conv2 and conv3): 1e-4 of the largest entry and >= 10x closer to
        the rounded oracle than the fp32 step;
      * stage-1 centres: median per-sample error <= 1e-3, max <= 2e-2; later predictions of samples whose yaw decode agrees:
        <= 1e-1; loss within 5e-3 (5e-2 with decode flips);
      * whole gradient: cosine >= 0.93 with the rounded oracle's (0.85 with flips) and >= 3x closer (1 - cos) than the fp32 step's
        gradient.  (Two max-pools -- over the k neighbours and over the points -- make this backbone's gradient far more sensitive
        to which row wins a near-tie than PointNet's: at these batch sizes the UNROUNDED fp64 oracle's gradient has cosine
        0.53 - 0.59 with the rounded oracle's; the engine's is at 0.958 - 0.962, every variable between 0.93 and 0.98.)"""
    cfg, spec, P32, d, du = _setup_dgcnn(N, B, std=std)
    us = [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")]
    stats = ["siamese/transformer1/embedding/conv2/bn/moving_mean", "siamese_1/transformer1/embedding/conv2/bn/moving_var",
             "siamese/transformer1/embedding/conv3/bn/moving_mean", "siamese_1/transformer1/embedding/conv3/bn/moving_var"]
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    res32 = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
    ema32 = {k: eng.get_variable(k) for k in stats}
    g32 = np.concatenate([eng.get_gradient(n).astype(np.float64).ravel() for n in R.trainable_names(spec)])
    eng.set_variables(P32)
    eng.set_option("train_matmul_bf16", 1)
    ep_ref, loss_ref, grads, ema_ref = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], bf16_lift=True)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
    assert res["loss"] != res32["loss"], "bf16 option had no effect"
    assert eng.get_option("last_train_kernel") & 6 == 6   # bit 1: bf16 operands, bit 2: dgcnn
    for k in stats:
        got, ref = eng.get_variable(k), ema_ref[k]
        e16, e32 = float(np.abs(got - ref).max()), float(np.abs(ema32[k] - ref).max())
        print(k, "err vs rounded oracle %.2e (fp32 step: %.2e), scale %.2e" % (e16, e32, np.abs(ref).max()))
        assert e16 <= 1e-4 * np.abs(ref).max() and e16 < 0.1 * e32, (k, e16, e32)
    nb = spec.num_bins
    flipped = np.zeros(B, bool)
    for k in ("pred_pc1angle_logits", "pred_pc2angle_logits"):
        flipped |= np.argmax(res[k][:, :nb], 1) != np.argmax(ep_ref[k][:, :nb], 1)
    print("decode flips vs the rounded oracle:", int(flipped.sum()), "of", B)
    assert flipped.sum() <= max(1, B // 8)
    for k in ep_ref:
        if k in ("pred_translations", "pred_remaining_angle_logits") and flipped.any():
            continue   # the pair head normalises over the batch: a flipped sample moves every row of its output
        per = np.abs(res[k] - ep_ref[k]).reshape(B, -1).max(1)[~flipped]
        print(k, "median %.2e max %.2e" % (np.median(per), per.max()))
        if "s1_" in k:
            assert np.median(per) <= 1e-3 and per.max() <= 2e-2, (k, per.max())
        assert per.max() <= 1e-1, (k, per.max())
    # (loss: 5.2e-3 measured at N = 128, B = 8 with the statistics 4e-6 from the oracle's -- the bound of the general-depth bf16 test)
    assert abs(res["loss"] - loss_ref) <= (5e-2 if flipped.any() else 1e-2) * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    g = np.concatenate([eng.get_gradient(n).astype(np.float64).ravel() for n in R.trainable_names(spec)])
    gr = np.concatenate([np.asarray(grads[n], np.float64).ravel() for n in R.trainable_names(spec)])
    cos = float(g @ gr / (np.linalg.norm(g) * np.linalg.norm(gr)))
    cos32 = float(g32 @ gr / (np.linalg.norm(g32) * np.linalg.norm(gr)))
    print("gradient cosine vs the rounded oracle: %.4f (the fp32 step's gradient: %.4f)" % (cos, cos32))
    assert cos >= (0.85 if flipped.any() else 0.93) and (1 - cos) < (0.7 if flipped.any() else 0.3) * (1 - cos32), (cos, cos32)
    eng.close()


@pytest.mark.parametrize("backbone", ["pointnet", "dgcnn"])
def test_negative_gammas(gpu_required, backbone):
    """BatchNorm gammas of mixed sign: the max-pools are taken as the extreme of sign(gamma)*z before the statistics
    exist (max for gamma >= 0, min for gamma < 0) -- over the points in both backbones, over the k neighbours in DGCNN.
    Forward, loss and every gradient against autograd with half of all gammas negated."""
    N, B = 128, 8
    cfg, spec, P32, d, du = (_setup_dgcnn if backbone == "dgcnn" else _setup)(N, B)
    rng = np.random.default_rng(11)
    for k in sorted(P32):
        if k.endswith("/gamma"):
            P32[k] = (P32[k] * rng.choice([-1.0, 1.0], size=P32[k].shape)).astype(np.float32)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    ep_ref, loss_ref, grads, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=eng.debug_train_decisions(B, relu=True))   # (pinned to this step's decisions and relu signs)
    for k in ep_ref:
        np.testing.assert_allclose(res[k], ep_ref[k], rtol=2e-4, atol=2e-4, err_msg=k)
    assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    gscale = max(float(np.abs(v).max()) for v in grads.values())
    bn_bias = set()
    for L in R.layer_table(spec):
        if L.bn:
            bn_bias.add((f"siamese/{L.name}" if L.siamese else L.name) + "/biases")
    bad, worst = {}, 0.0
    for name in R.trainable_names(spec):
        if name in bn_bias:
            continue
        g = eng.get_gradient(name).astype(np.float64)
        ref = grads[name].reshape(g.shape)
        err = float(np.abs(g - ref).max())
        worst = max(worst, err / (float(np.abs(ref).max()) + 1e-6 * gscale))
        if err > 3e-3 * float(np.abs(ref).max()) + 1e-5 * gscale:
            bad[name] = (err, float(np.abs(ref).max()))
    print(backbone, "negative gammas: worst relative gradient error", worst)
    assert not bad, bad
    eng.close()


def test_gradients_wide_first_layers(gpu_required):
    """C1 = C2 = 128 (the widest the training path accepts): the weight-gradient blocks no longer fit the registers of pass B1, so
    pass B2 accumulates U2 / Gram(h1) per tile, pass B1 stores dy1 and pass B0 runs (the generic kernel instantiations)."""
    N, B = 128, 8
    cfg = small_cfg(N=N, nb=12, s1=(128, 128, 96), s2=(128, 128, 128), emb=(128, 128, 160), fc=(64, 32))
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=5)
    d = R.synth_pairs(B, N, seed=5, dtype=np.float32)
    rng = np.random.default_rng(5)
    du = {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    ep_ref, loss_ref, grads, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=eng.debug_train_decisions(B, relu=True))   # (pinned to this step's decisions and relu signs)
    for k in ep_ref:
        np.testing.assert_allclose(res[k], ep_ref[k], rtol=2e-4, atol=2e-4, err_msg=k)
    gscale = max(float(np.abs(v).max()) for v in grads.values())
    bn_bias = {(f"siamese/{L.name}" if L.siamese else L.name) + "/biases" for L in R.layer_table(spec) if L.bn}
    bad, worst = {}, 0.0
    for name in R.trainable_names(spec):
        if name in bn_bias:
            continue
        g = eng.get_gradient(name).astype(np.float64)
        ref = grads[name].reshape(g.shape)
        err = float(np.abs(g - ref).max())
        worst = max(worst, err / (float(np.abs(ref).max()) + 1e-6 * gscale))
        if err > 3e-3 * float(np.abs(ref).max()) + 1e-5 * gscale:
            bad[name] = (err, float(np.abs(ref).max()))
    print("wide first layers: worst relative gradient error", worst)
    assert not bad, bad
    eng.close()


def _grad_check(eng, spec, grads, tol, skip_bn_bias=True):
    gscale = max(float(np.abs(v).max()) for v in grads.values())
    bn_bias = {(f"siamese/{L.name}" if L.siamese else L.name) + "/biases" for L in R.layer_table(spec) if L.bn}
    bad, worst = {}, 0.0
    for name in R.trainable_names(spec):
        g = eng.get_gradient(name).astype(np.float64)
        ref = grads[name].reshape(g.shape)
        if name in bn_bias:
            assert np.abs(g).max() == 0.0 and np.abs(ref).max() < 1e-9 * gscale, name
            continue
        err = float(np.abs(g - ref).max())
        worst = max(worst, err / (float(np.abs(ref).max()) + 1e-6 * gscale))
        if err > tol * float(np.abs(ref).max()) + 1e-5 * gscale:
            bad[name] = (err, float(np.abs(ref).max()))
    return bad, worst


GENERAL_DEPTH = {
    # the reference's configs/default.json layer structure (five-layer s2 / embedding backbones, a wide first layer in s1), narrowed
    "default_json_like": dict(s1=(128, 128, 160), s2=(32, 32, 32, 64, 128), emb=(32, 32, 32, 64, 160)),
    # two and four layers, widths that are not multiples of 32, a hidden width above 128
    "odd_shapes": dict(s1=(24, 40), s2=(16, 136, 48, 72), emb=(8, 16, 24, 200)),
    # fused-tail shapes other than default.json's: three layers with an odd first width, a 96-wide and a 32-wide layer in front of the tail
    "tail_shapes": dict(s1=(24, 96, 224), s2=(16, 40, 32, 96), emb=(40, 128, 256)),
}


@pytest.mark.parametrize("case,N,B,tail", [("default_json_like", 100, 6, 1), ("odd_shapes", 128, 5, 1), ("default_json_like", 128, 8, 1),
                                           ("default_json_like", 100, 6, 0), ("default_json_like", 128, 8, 0),
                                           ("tail_shapes", 100, 6, 1), ("tail_shapes", 128, 5, 0)])
def test_general_depth_backbones_train(gpu_required, case, N, B, tail):
    """models/tp8.py:49-59 builds a conv layer per entry of `layer_sizes`, and the reference's configs/default.json:13-15 uses five.
    Stages outside the specialised three-layer shape run the layer-by-layer path (csrc/kernels_train_generic.h): train-mode
    predictions, loss, EMA updates and every gradient against torch autograd (fp64), same criteria as the three-layer tests.
    N = 100 gives 64-row tiles that end inside a tower (B * N = 600 rows) and a partial last tile.
    (Not every instance is comparable at this tolerance: at N = 64, B = 16, seed 9 two pooled maxima of one tower are 1.4e-5 apart --
    the size of the fp32 forward error -- and a swapped arg-max row re-routes a gradient that is 17 % of one weight column; the fp32
    evaluation of the oracle itself shows the same effect in the other tower.  tools/grad_report_generic.py prints both.)
    tail: option "train_fused_tail" -- 1 (default): a stage whose last two widths fit the fused kernels (default_json_like's s2 and
    embedding) runs only the layers in front of them layer by layer and the last layer on phase 3 / pass B2 with given features
    (last_train_kernel bit 16); 0: every layer layer by layer.  Both against the same oracle at the same tolerances."""
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), **GENERAL_DEPTH[case])
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=9)
    d = R.synth_pairs(B, N, seed=9, dtype=np.float32)
    rng = np.random.default_rng(9)
    du = {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    assert eng.get_option("train_fused_tail") == 1
    eng.set_option("train_fused_tail", tail)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    ep_ref, loss_ref, grads, ema_ref = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=eng.debug_train_decisions(B, relu=True))   # (pinned to this step's decisions and relu signs)
    assert eng.get_option("last_train_kernel") & 8, "the general-depth path did not run"
    assert bool(eng.get_option("last_train_kernel") & 16) == (tail == 1 and case != "odd_shapes"), eng.get_option("last_train_kernel")
    for k in ep_ref:
        np.testing.assert_allclose(res[k], ep_ref[k], rtol=2e-4, atol=2e-4, err_msg=k)
    assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    for k, v in ema_ref.items():
        np.testing.assert_allclose(eng.get_variable(k), v, rtol=1e-4, atol=1e-5, err_msg=k)
    bad, worst = _grad_check(eng, spec, grads, 3e-3 if B >= 8 else 1e-2)
    print(case, N, B, "general-depth path: loss", res["loss"], loss_ref, "worst relative gradient error", worst)
    assert not bad, bad
    # and a full optimiser step on it
    r = eng.train_step(d["pcs1"], d["pcs2"], d)
    assert r["step"] == 1 and np.isfinite(r["loss"])
    eng.close()


@pytest.mark.parametrize("backbone,bf16,widths", [("pointnet", 0, "std"), ("pointnet", 1, "std"), ("dgcnn", 0, "std"), ("dgcnn", 1, "std"),
                                                  ("pointnet", 0, "deep"), ("dgcnn", 0, "deep")])
def test_training_step_is_bitwise_reproducible(gpu_required, backbone, bf16, widths):
    """No atomics on floats and fixed summation orders everywhere in the training path: the same batch twice on one engine, and once
    on a second engine, gives bit-identical loss, predictions and gradients -- at a size with hundreds of workgroups in flight
    (B = 48 pairs, N = 320: partial last tile), so that a missing barrier or a read of a buffer another workgroup is still writing
    shows up as a difference.  Covers the fused PointNet kernels (fp32 / bf16), the DGCNN edge kernels (list form / dense bf16 form)
    and the layer-by-layer paths."""
    B, N = 48, 320
    if widths == "std":
        w = STD
    elif backbone == "dgcnn":
        w = dict(s1=(32, 32, 64, 96), s2=(48, 96, 128), emb=(64, 160))
    else:
        w = dict(s1=(128, 128, 160), s2=(32, 32, 32, 64, 128), emb=(32, 32, 32, 64, 160))
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), backbone=backbone, **w)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=21)
    d = R.synth_pairs(B, N, seed=21, dtype=np.float32)
    rng = np.random.default_rng(21)
    du = [rng.uniform(size=(B, 32)).astype(np.float32) for _ in range(5)]
    runs = []
    for e in range(2):
        eng = alignnet3d.Engine(cfg)
        eng.set_variables(P32)
        if bf16:
            eng.set_option("train_matmul_bf16", 1)
        for rep in range(2 if e == 0 else 1):
            eng.set_variables(P32)   # (the EMA shadows too)
            res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, du)
            runs.append((res, {n: eng.get_gradient(n).copy() for n in R.trainable_names(spec)}))
        eng.close()
    res0, g0 = runs[0]
    assert np.isfinite(res0["loss"])
    for res, g in runs[1:]:
        assert res["loss"] == res0["loss"], (res["loss"], res0["loss"])
        for k in alignnet3d.OUTPUT_NAMES:
            np.testing.assert_array_equal(res[k], res0[k], err_msg=k)
        for n in g0:
            np.testing.assert_array_equal(g[n], g0[n], err_msg=n)


@pytest.mark.parametrize("N,B,bf16", [(200, 16, 0), (384, 12, 0), (96, 16, 0), (136, 16, 0), (200, 8, 0), (264, 16, 0), (72, 16, 0), (201, 12, 0), (135, 10, 0),
                                      (200, 16, 1), (384, 12, 1), (96, 16, 1), (264, 16, 1), (135, 10, 1),
                                      (200, 8, -1), (136, 6, -1), (96, 8, -1)])
def test_phase3_tile_shapes_agree(gpu_required, N, B, bf16):
    """The forward's phase 3 on 128-point tiles (default for the shipped widths 64 / 128: kernels_train_fwd_wide.h) against the same
    phase on 64-point tiles (option train_phase3_tile64): the MFMA k-order is the same, so the lift's values -- hence the pooled
    extremes -- are bit-identical; only the grouping of the column sums of h2 differs (fp32 partial sums per lane, added in fp64), which
    the small-batch statistics amplify to ~1e-5 in the predictions: bounds a decade below the ones against the oracle.
    N = 200: partial last tile in both shapes (72 / 8 rows); N = 96: a cloud smaller than one wide tile.
    bf16 = 1 (train_matmul_bf16): the pipelined kernel train_fwd_phase3_wide_bf16 against train_fwd_phase23<3, true, false, 64, 128>; the
    rounded h2 and the lift are bit-identical again, but a 1e-7 difference in a later stage's input can fall on the other side of a bf16
    rounding boundary (4e-3 of that element), so the bounds are those of two bf16 runs, not of two fp32 runs.
    bf16 = -1: the dgcnn backbone in fp32, whose point conv runs the same phase on the stored pooled edge features
    (train_fwd_phase3_wide<true> against train_fwd_phase23<3, false, true, 64, 128>): nothing but the arg-max among copies of a
    cloud's last row can differ."""
    dg = bf16 < 0
    bf16 = max(bf16, 0)
    cfg, spec, P32, d, du = _setup_dgcnn(N, B, std=True) if dg else _setup(N, B, std=True)
    ul = [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")]
    out = []
    for t64 in (0, 1):
        eng = alignnet3d.Engine(cfg)
        eng.set_variables(P32)
        eng.set_option("train_phase3_tile64", t64)
        eng.set_option("train_matmul_bf16", bf16)
        eng.set_option("pn_cloud_parts", 1)   # one workgroup per cloud in both: the tile shapes are what is compared (the split: test_ab_variants_gpu.py)
        assert eng.get_option("train_phase3_tile64") == t64
        res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, ul)
        out.append((res, {n: eng.get_gradient(n).copy() for n in R.trainable_names(spec)},
                    {k: eng.get_variable(k).copy() for k, _, tr in eng.variables() if not tr}))
        eng.close()
    (ra, ga, ea), (rb, gb, eb) = out
    lt, pt, et = (2e-3, 5e-3, 1e-3) if bf16 else (2e-5, 3e-5, 1e-5)
    assert abs(ra["loss"] - rb["loss"]) <= lt * max(1.0, abs(rb["loss"]))
    for k in alignnet3d.OUTPUT_NAMES:
        np.testing.assert_allclose(ra[k], rb[k], rtol=pt, atol=pt, err_msg=k)
    for k in ea:
        # (absolute part: a head layer's moving mean is a sum of unit-scale pre-activations that nearly cancels -- measured 1.4e-6 on a mean of 0.015)
        np.testing.assert_allclose(ea[k], eb[k], rtol=et, atol=et * 0.5, err_msg=k)
    gscale = max(float(np.abs(v).max()) for v in gb.values())
    # gradients: a 1e-6 difference in stage 1's output moves the points of the later stages, and a max-pool near-tie that falls the other
    # way re-routes one channel's gradient.  Measured over these nine shapes: relative L2 of the whole gradient 4e-6 .. 5e-5 in seven of
    # them, 7e-4 and 4e-3 in two (N = 200 at B = 16 but not at B = 8; N = 264) -- data-dependent flips, not a tile-remainder effect.
    num = sum(float(((ga[n].astype(np.float64) - gb[n]) ** 2).sum()) for n in ga)
    den = sum(float((gb[n].astype(np.float64) ** 2).sum()) for n in ga)
    print("relative L2 difference of the whole gradient between the tile shapes:", (num / den) ** 0.5)
    assert (num / den) ** 0.5 <= (1e-1 if bf16 else 1e-2)


DGCNN_GENERAL = {
    # models/tp8.py:38-41 builds one edge conv per entry of sizes[:-1]: three edge convs, an odd first width, a single edge conv
    "deep_odd": dict(s1=(32, 32, 64, 96), s2=(48, 96, 128), emb=(64, 160)),
    # a specialised stage (32, 64, .) between two layer-by-layer ones: the stage glue folded into the specialised edge kernels must
    # not leak into the stage in front of it
    "mixed": dict(s1=(24, 40, 96), s2=(32, 64, 128), emb=(16, 136, 48, 160)),
}


@pytest.mark.parametrize("case,N,B", [("deep_odd", 96, 6), ("mixed", 128, 5), ("deep_odd", 128, 8)])
def test_dgcnn_general_widths_and_depth_train(gpu_required, case, N, B):
    """DGCNN stages outside the specialised [C1 in {32, 64}, C2 in {64, 128}, C3] shape train layer by layer over the B N k edge rows
    (csrc/kernels_train_generic.h: gen_edge_kernel / gen_layer1e_* + the general-depth kernels; max over k and over N through
    gen_pool_*): predictions, loss, EMA and every gradient against torch autograd (fp64), the three-layer DGCNN tests' criteria.
    The eval-mode forward of the same engine (the fused dgcnn kernels take any depth) against the oracle as well."""
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), backbone="dgcnn", **DGCNN_GENERAL[case])
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=11)
    d = R.synth_pairs(B, N, seed=11, dtype=np.float32)
    rng = np.random.default_rng(11)
    du = {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    ep_ref, loss_ref, grads, ema_ref = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=eng.debug_train_decisions(B, relu=True))   # (pinned to this step's decisions and relu signs)
    assert eng.get_option("last_train_kernel") & 12 == 12, "the layer-by-layer dgcnn path did not run"
    for k in ep_ref:
        np.testing.assert_allclose(res[k], ep_ref[k], rtol=2e-4, atol=2e-4, err_msg=k)
    assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    for k, v in ema_ref.items():
        np.testing.assert_allclose(eng.get_variable(k), v, rtol=1e-4, atol=1e-5, err_msg=k)
    # (k-max per point and channel: the fp32 evaluation of the oracle itself is 1e-2 .. 3e-2 away from the fp64 one where a near-tie
    # routes a gradient to another edge row -- test_dgcnn_gradients_match_autograd; bound: twice the fp32 oracle's own error)
    _, _, g32, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], dt=np.float32, pinned=eng.debug_train_decisions(B, relu=True))
    gs = max(float(np.abs(v).max()) for v in grads.values())
    rel32 = max(float(np.abs(g32[k].astype(np.float64) - grads[k]).max()) / (float(np.abs(grads[k]).max()) + 1e-5 * gs) for k in grads)
    bad, worst = _grad_check(eng, spec, grads, min(max(3e-3 if B >= 8 else 1e-2, 2.0 * rel32), 8e-2))   # (capped: "mixed" at B = 5 has an fp32-oracle error of 0.26)
    print(case, N, B, "dgcnn layer-by-layer path: loss", res["loss"], loss_ref, "worst relative gradient error", worst, "fp32 oracle vs fp64 oracle:", rel32)
    assert not bad, bad
    r = eng.train_step(d["pcs1"], d["pcs2"], d)
    assert r["step"] == 1 and np.isfinite(r["loss"])
    # a smaller batch on the same workspace (tiles / slabs of THIS call, not of the capacity)
    d2 = R.synth_pairs(B - 2, N, seed=12, dtype=np.float32)
    fresh = alignnet3d.Engine(cfg)
    fresh.set_variables({k: eng.get_variable(k) for k in P32})
    r2 = eng.train_forward_backward(d2["pcs1"], d2["pcs2"], d2, [du[k][: B - 2] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    r3 = fresh.train_forward_backward(d2["pcs1"], d2["pcs2"], d2, [du[k][: B - 2] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    assert abs(r2["loss"] - r3["loss"]) <= 1e-6 * max(1.0, abs(r3["loss"])), (r2["loss"], r3["loss"])
    gs = max(float(np.abs(fresh.get_gradient(n)).max()) for n in R.trainable_names(spec))
    for name in R.trainable_names(spec):
        a, b = eng.get_gradient(name).astype(np.float64), fresh.get_gradient(name).astype(np.float64)
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-7 * gs, ("reused vs fresh engine", name, float(np.abs(a - b).max()), float(np.abs(b).max()))
    fresh.close()
    eng.close()


@pytest.mark.parametrize("tail", [1, 0])
def test_general_depth_smaller_batch_after_larger(gpu_required, tail):
    """One engine, B = 8 and then B = 5 (the workspace keeps the larger capacity): the layer-by-layer kernels must walk the tiles of
    THIS call's B * N rows -- taking the tile count from the workspace capacity ran tiles past the batch's end, whose negative row
    counts corrupted the batch statistics and EMA of every general-depth layer (round-2 advisor finding)."""
    N = 128
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), **GENERAL_DEPTH["default_json_like"])
    eng = None
    for B in (8, 5):
        cfg["training"]["batch_size"] = B
        spec, P32 = oracle_params(cfg, seed=9)
        d = R.synth_pairs(B, N, seed=9, dtype=np.float32)      # (the instances test_general_depth_backbones_train uses: well-conditioned max-pools)
        rng = np.random.default_rng(9)
        du = {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
        if eng is None:
            eng = alignnet3d.Engine(cfg)
            eng.set_option("train_fused_tail", tail)
        eng.set_variables(P32)      # (the EMA shadows too: every call starts from the same state as its oracle)
        res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
        ep_ref, loss_ref, grads, ema_ref = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=eng.debug_train_decisions(B, relu=True))   # (pinned to this step's decisions and relu signs)
        assert eng.get_option("last_train_kernel") & 8
        for k in ep_ref:
            np.testing.assert_allclose(res[k], ep_ref[k], rtol=2e-4, atol=2e-4, err_msg="B=%d %s" % (B, k))
        assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (B, res["loss"], loss_ref)
        for k, v in ema_ref.items():
            np.testing.assert_allclose(eng.get_variable(k), v, rtol=1e-4, atol=1e-5, err_msg="B=%d %s" % (B, k))
        if B == 8:
            bad, worst = _grad_check(eng, spec, grads, 3e-3)
            assert not bad, (B, bad)
        else:
            # the smaller batch on the engine whose workspace was carved for the larger one must give what a fresh engine gives (five-row
            # batch statistics make the comparison with fp64 autograd a conditioning lottery; engine against engine is exact up to the
            # order of a few fp32 sums)
            fresh = alignnet3d.Engine(cfg)
            fresh.set_option("train_fused_tail", tail)
            fresh.set_variables(P32)
            res_f = fresh.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
            for k in ep_ref:
                np.testing.assert_allclose(res[k], res_f[k], rtol=1e-6, atol=1e-6, err_msg="reused vs fresh engine: " + k)
            gs = max(float(np.abs(fresh.get_gradient(n)).max()) for n in R.trainable_names(spec))
            for n in R.trainable_names(spec):
                a, b = eng.get_gradient(n).astype(np.float64), fresh.get_gradient(n).astype(np.float64)
                assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 1e-7 * gs, ("reused vs fresh engine", n, float(np.abs(a - b).max()), float(np.abs(b).max()))
            fresh.close()
            bad, worst = _grad_check(eng, spec, grads, 1e-1)
            assert not bad, (B, bad)
    eng.close()


def test_general_depth_bf16_tail_matches_rounded_oracle(gpu_required):
    """"train_matmul_bf16" on general-depth backbones (default.json's five-layer s2 / embedding; four layers in s1): they take bf16
    operands only in their last layer -- the fused tail (phase 3 on given features with the
    features rounded while they are staged; pass B2 on given features with its dense product on bf16); the layers in front of it stay fp32.  The oracle rounds
    exactly those layers (TorchTp8.bf16_conv_layers).  Criteria of the other bf16 tests: batch statistics of the rounded last layer
    to 1e-4 of their scale and >= 10x closer than the fp32 step, loss within 1e-2 (5e-2 with decode flips; three tails in a row
    feed each other's inputs here), gradient cosine >= 0.97 (0.85) and >= 3x closer (1 - cos) than the fp32 step's."""
    B, N = 16, 128
    # (stage 1 is given four layers here so that a fused tail sees inputs identical to the oracle's: stages 2 and 3 start from
    #  stage 1's predicted centre / decoded yaw, which already carry the bf16 difference)
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), s1=(16, 32, 64, 128), s2=(32, 32, 32, 64, 128), emb=(32, 32, 32, 64, 160))
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=13)
    d = R.synth_pairs(B, N, seed=13, dtype=np.float32)
    rng = np.random.default_rng(13)
    du = {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
    us = [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")]
    stats = ["siamese/transformer1/embedding/conv4/bn/moving_mean", "siamese_1/transformer1/embedding/conv4/bn/moving_var"]
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    res32 = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
    ema32 = {k: eng.get_variable(k) for k in stats}
    g32 = np.concatenate([eng.get_gradient(n).astype(np.float64).ravel() for n in R.trainable_names(spec)])
    eng.set_variables(P32)
    eng.set_option("train_matmul_bf16", 1)
    ep_ref, loss_ref, grads, ema_ref = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], bf16_lift=True)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
    assert eng.get_option("last_train_kernel") & 26 == 26   # bf16 operands, general depth, fused tail
    assert res["loss"] != res32["loss"]
    for k in stats:
        got, ref = eng.get_variable(k), ema_ref[k]
        e16, e32 = float(np.abs(got - ref).max()), float(np.abs(ema32[k] - ref).max())
        print(k, "err vs rounded oracle %.2e (fp32 step: %.2e), scale %.2e" % (e16, e32, np.abs(ref).max()))
        assert e16 <= 1e-4 * np.abs(ref).max() and e16 < 0.1 * e32, (k, e16, e32)
    nb = spec.num_bins
    flipped = np.zeros(B, bool)
    for k in ("pred_pc1angle_logits", "pred_pc2angle_logits"):
        flipped |= np.argmax(res[k][:, :nb], 1) != np.argmax(ep_ref[k][:, :nb], 1)
    clean = not flipped.any()
    print("decode flips:", int(flipped.sum()), "loss", res["loss"], loss_ref, "fp32 step's", res32["loss"])
    assert flipped.sum() <= max(1, B // 8)
    assert abs(res["loss"] - loss_ref) <= (1e-2 if clean else 5e-2) * max(1.0, abs(loss_ref))
    g = np.concatenate([eng.get_gradient(n).astype(np.float64).ravel() for n in R.trainable_names(spec)])
    gr = np.concatenate([np.asarray(grads[n], np.float64).ravel() for n in R.trainable_names(spec)])
    cos = float(g @ gr / (np.linalg.norm(g) * np.linalg.norm(gr)))
    cos32 = float(g32 @ gr / (np.linalg.norm(g32) * np.linalg.norm(gr)))
    print("gradient cosine vs the rounded oracle: %.4f (fp32 step's: %.4f)" % (cos, cos32))
    assert cos > (0.97 if clean else 0.85) and (1 - cos) < (0.3 if clean else 0.7) * (1 - cos32), (cos, cos32)
    eng.close()


def test_fused_tail_option_switches_in_place(gpu_required):
    """"train_fused_tail" changes how the training workspace is carved: switching it on a live engine re-carves on the next step, and
    the two settings agree with each other to summation-order noise (same parameters, same batch, same dropout uniforms)."""
    cfg = small_cfg(N=128, nb=12, fc=(64, 32), **GENERAL_DEPTH["default_json_like"])
    cfg["training"]["batch_size"] = 8
    spec, P32 = oracle_params(cfg, seed=11)
    d = R.synth_pairs(8, 128, seed=11, dtype=np.float32)
    rng = np.random.default_rng(11)
    us = [rng.uniform(size=(8, 32)).astype(np.float32) for _ in range(5)]
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    out = {}
    for tail in (1, 0, 1):
        eng.set_variables(P32)
        eng.set_option("train_fused_tail", tail)
        res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
        assert bool(eng.get_option("last_train_kernel") & 16) == bool(tail)
        g = np.concatenate([eng.get_gradient(n).astype(np.float64).ravel() for n in R.trainable_names(spec)])
        if tail in out:
            np.testing.assert_array_equal(out[tail][1], g)   # back on the first setting: bit-identical
        out[tail] = (res["loss"], g)
    assert abs(out[0][0] - out[1][0]) <= 1e-5 * max(1.0, abs(out[0][0]))
    err = np.abs(out[0][1] - out[1][1]).max() / np.abs(out[0][1]).max()
    print("fused tail vs layer by layer: loss %.7f / %.7f, worst gradient difference %.2e of the largest entry" % (out[1][0], out[0][0], err))
    assert err <= 5e-5
    eng.close()


def test_reference_default_config_trains(gpu_required):
    """The merged reference default config itself (configs/default.json: s1 [128,128,256], s2 / embedding [64,64,64,128,1024], 36
    bins, no inverted angles) at N = 256: 80 Adam steps on fresh batches reduce the loss (first ten vs last ten steps: 0.64 -> 0.42
    on two seeds and two builds; the trajectory itself is chaotic -- a 1e-6 change in a gradient's summation order moves the loss of
    step 3 by a percent -- so the criterion is a window mean, not a step), eval afterwards is finite."""
    cfg = alignnet3d.default_model_config()
    o = cfg["model"]["options"]
    o["s1transformer"] = [[128, 128, 256], [[512, 256], 0.7]]
    o["s2transformer"] = [[64, 64, 64, 128, 1024], [[512, 256], 0.7]]
    o["embedding"] = [64, 64, 64, 128, 1024]
    o["early_stage_factor"] = 0.1
    cfg["model"]["angles"] = {"num_bins": 36, "accept_inverted_angle": False}
    cfg["model"]["num_points"] = 256
    cfg["training"]["batch_size"] = 32
    cfg["training"]["learning_rate"] = 0.002
    cfg["data"]["ntrain"] = 3200
    eng = alignnet3d.Engine(cfg, seed=3)
    losses = []
    for k in range(80):
        d = R.synth_pairs(32, 256, seed=3000 + k, dtype=np.float32)
        losses.append(eng.train_step(d["pcs1"], d["pcs2"], d)["loss"])
    assert eng.get_option("last_train_kernel") & 8
    held = R.synth_pairs(32, 256, seed=997, dtype=np.float32)
    pred = eng.forward(held["pcs1"], held["pcs2"])["pred_translations"]
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print("default.json widths: mean loss first / last 10 steps", first, last)
    assert np.all(np.isfinite(losses)) and np.isfinite(pred).all() and last < 0.8 * first, (first, last)
    eng.close()


@pytest.mark.parametrize("backbone,bf16,std", [("pointnet", 0, False), ("pointnet", 0, True), ("pointnet", 1, True), ("dgcnn", 0, True), ("dgcnn", 1, True)])
def test_sync_bn_with_identical_virtual_ranks_reproduces_local_step(gpu_required, backbone, bf16, std):
    """Option "sync_bn": every batch sum behind a BatchNorm (forward moments, the Gram / column-sum matrices the layer identities use,
    the backward's dbeta / dgamma totals, the heads' row statistics) is added over the data-parallel ranks and divided by the GLOBAL
    count -- the reference's single-device semantics at the global batch (utils/tf_util.py:474).  Real ranks need more than one GPU;
    the test hook "sync_bn_emulate_world" = 2 stands for two ranks holding the SAME shard (each all-reduce becomes x 2, exact in
    binary floating point): mean and variance are then the shard's own, bit for bit, so predictions, loss, EMA shadows and every gradient must equal the plain local-BN step --
    which they only do if every count carries its x world and every globally-summed gradient term its 1 / world."""
    N, B = 128, 6
    cfg, spec, P32, d, du = (_setup_dgcnn(N, B, std=std) if backbone == "dgcnn" else _setup(N, B, std=std))
    us = [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")]
    out = {}
    for mode in (0, 1):
        eng = alignnet3d.Engine(cfg)
        eng.set_variables(P32)
        eng.set_option("train_matmul_bf16", bf16)
        if mode:
            eng.set_option("sync_bn", 1)
            eng.set_option("sync_bn_emulate_world", 2)
        res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
        grads = {n: eng.get_gradient(n).astype(np.float64) for n in R.trainable_names(spec)}
        ema = {k: eng.get_variable(k) for k, _, tr in eng.variables() if not tr}
        out[mode] = (res, grads, ema)
        eng.close()
    (r0, g0, e0), (r1, g1, e1) = out[0], out[1]
    # x 3 and / 3 round differently from the single sum: differences are rounding-sized in fp32 (amplified by six-row batch statistics
    # in the heads) and bf16-ulp-sized where a value sits on a rounding boundary of the bf16 operands; a missing x world or
    # 1 / world would be a factor of 3 in a statistic or a gradient term
    ptol, ltol, gtol = 1e-6, 1e-6, 1e-6   # (x 2 and / 2 are exact: nothing but a wrong factor can move a result)
    assert abs(r0["loss"] - r1["loss"]) <= ltol * max(1.0, abs(r0["loss"]))
    for k in ("pred_translations", "pred_remaining_angle_logits", "pred_s2_pc1centers", "pred_pc2angle_logits"):
        np.testing.assert_allclose(r1[k], r0[k], rtol=ptol, atol=ptol, err_msg=k)
    for k in e0:
        np.testing.assert_allclose(e1[k], e0[k], rtol=10 * ltol, atol=ltol, err_msg=k)
    gs = max(float(np.abs(v).max()) for v in g0.values())
    worst = 0.0
    for n in g0:
        err = float(np.abs(g1[n] - g0[n]).max())
        worst = max(worst, err / (float(np.abs(g0[n]).max()) + 1e-6 * gs))
        assert err <= gtol * float(np.abs(g0[n]).max()) + 1e-2 * gtol * gs, (n, err, float(np.abs(g0[n]).max()))
    ga, gb = np.concatenate([g0[n].ravel() for n in g0]), np.concatenate([g1[n].ravel() for n in g0])
    cos = float(ga @ gb / (np.linalg.norm(ga) * np.linalg.norm(gb)))
    assert cos > 0.9999999, cos
    print(backbone, "bf16" if bf16 else "fp32", "sync_bn (2 identical virtual ranks) vs local step: worst relative gradient difference %.2e, cosine %.7f" % (worst, cos))


@pytest.mark.parametrize("backbone,tail", [("pointnet", 1), ("pointnet", 0), ("dgcnn", 1)])
def test_sync_bn_general_depth_with_identical_virtual_ranks(gpu_required, backbone, tail):
    """The same check for stages that train layer by layer (kernels_train_generic.h: any depth / widths, the reference's own
    configs/default.json has five conv layers per backbone): gen_stat_finish forms this rank's sum, the all ranks' mean, this rank's
    squared differences from THAT mean and the statistics with the global count in three launches around two all-reduces,
    gen_bn_bwd_finish the backward coefficients from all ranks' (dbeta, dgamma).  PointNet: a hybrid stage (48, 96, 160), a five-layer
    stage with a fused tail and a stage no fused kernel fits (40, 72, 104); with train_fused_tail off every stage runs layer by layer.
    dgcnn: three edge convs, an odd width, a single edge conv."""
    N, B = 128, 6
    if backbone == "dgcnn":
        w = dict(s1=(32, 32, 64, 96), s2=(48, 96, 128), emb=(64, 160))
    else:
        w = dict(s1=(48, 96, 160), s2=(32, 32, 32, 64, 128), emb=(40, 72, 104))
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), backbone=backbone, **w)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=5)
    d = R.synth_pairs(B, N, seed=5, dtype=np.float32)
    rng = np.random.default_rng(5)
    us = [rng.uniform(size=(B, 32)).astype(np.float32) for _ in range(5)]
    out = {}
    for mode in (0, 1):
        eng = alignnet3d.Engine(cfg)
        eng.set_variables(P32)
        eng.set_option("train_fused_tail", tail)
        if mode:
            eng.set_option("sync_bn", 1)
            eng.set_option("sync_bn_emulate_world", 2)
        res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
        assert eng.get_option("last_train_kernel") & 8
        out[mode] = (res, {n: eng.get_gradient(n).astype(np.float64) for n in R.trainable_names(spec)},
                     {k: eng.get_variable(k) for k, _, tr in eng.variables() if not tr})
        eng.close()
    (r0, g0, e0), (r1, g1, e1) = out[0], out[1]
    assert abs(r0["loss"] - r1["loss"]) <= 1e-6 * max(1.0, abs(r0["loss"]))
    for k in ("pred_translations", "pred_remaining_angle_logits", "pred_s2_pc1centers", "pred_pc2angle_logits"):
        np.testing.assert_allclose(r1[k], r0[k], rtol=1e-6, atol=1e-6, err_msg=k)
    for k in e0:
        np.testing.assert_allclose(e1[k], e0[k], rtol=1e-5, atol=1e-6, err_msg=k)
    gs = max(float(np.abs(v).max()) for v in g0.values())
    for n in g0:
        err = float(np.abs(g1[n] - g0[n]).max())
        assert err <= 1e-6 * float(np.abs(g0[n]).max()) + 1e-8 * gs, (n, err, float(np.abs(g0[n]).max()))


@pytest.mark.parametrize("backbone,bf16", [("pointnet", 0), ("pointnet", 1), ("dgcnn", 0)])
def test_global_loss_with_identical_virtual_ranks(gpu_required, backbone, bf16):
    """Option "global_loss" (with "sync_bn"): end points and labels are all-gathered and the reference's loss -- whose [B, B] broadcast
    terms (models/tp8.py:279,327) and whole-batch tf.cond (:288) couple all samples -- is evaluated on the global batch; each rank keeps
    its rows of the gradient, the gradient all-reduce sums.  Two identical virtual ranks ("sync_bn_emulate_world" = 2: every gather
    is two copies): the global batch is the shard twice, so every mean in the loss is the shard's own, the loss (divided by the
    global B) is HALF the local step's, and this rank's share of the gradient a QUARTER of the local step's gradient (each sample
    appears twice in means over 2B rows, and the loss carries 1 / (2B)) -- up to the order of the fp64 sums inside the loss."""
    N, B = 128, 6
    cfg, spec, P32, d, du = (_setup_dgcnn(N, B, std=True) if backbone == "dgcnn" else _setup(N, B, std=True))
    us = [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")]
    out = {}
    for mode in (0, 1):
        eng = alignnet3d.Engine(cfg)
        eng.set_variables(P32)
        eng.set_option("train_matmul_bf16", bf16)
        if mode:
            eng.set_option("sync_bn", 1); eng.set_option("global_loss", 1); eng.set_option("sync_bn_emulate_world", 2)
        res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
        out[mode] = (res, {n: eng.get_gradient(n).astype(np.float64) for n in R.trainable_names(spec)})
        eng.close()
    (r0, g0), (r1, g1) = out[0], out[1]
    assert abs(r1["loss"] - 0.5 * r0["loss"]) <= 1e-5 * abs(r0["loss"]), (r0["loss"], r1["loss"])
    for k in ("pred_translations", "pred_remaining_angle_logits"):
        np.testing.assert_array_equal(r1[k], r0[k])
    gs = max(float(np.abs(v).max()) for v in g0.values())
    # fp32: every tensor to 1e-6 of its largest entry (measured 9e-7; tensors whose exact gradient is zero carry 1e-6-sized noise: the
    # absolute floor).  bf16 operands: 2 - 4e-3 on the hidden layers of stage 1 (measured; the quarter-sized gradient rounds
    # differently on its way through the bf16 dy2 / S tiles), bound 1e-2.
    rtol = 1e-2 if bf16 else 1e-5
    worst = 0.0
    for n in g0:
        err = float(np.abs(g1[n] - 0.25 * g0[n]).max())
        if np.abs(g0[n]).max() > 1e-4 * gs:
            worst = max(worst, err / (0.25 * float(np.abs(g0[n]).max())))
        assert err <= 0.25 * (rtol * float(np.abs(g0[n]).max()) + 1e-6 * gs), (n, err, float(np.abs(g0[n]).max()))
    print(backbone, "bf16" if bf16 else "fp32", "global_loss (2 identical virtual ranks): loss ratio %.7f, worst relative deviation of 4 x gradient %.2e" % (r1["loss"] / r0["loss"], worst))


PINNED_CASES = {
    # name: (backbone, widths, N, B, bf16, tail)
    "pointnet": ("pointnet", dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(32, 64, 160)), 256, 16, 0, 1),
    "pointnet_std": ("pointnet", STD, 192, 12, 0, 1),
    "pointnet_std_bf16": ("pointnet", STD, 192, 48, 1, 1),
    "pointnet_deep_tail": ("pointnet", GENERAL_DEPTH["default_json_like"], 128, 8, 0, 1),
    "pointnet_deep_layerwise": ("pointnet", GENERAL_DEPTH["odd_shapes"], 128, 5, 0, 0),
    "dgcnn": ("dgcnn", dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(64, 128, 160)), 128, 8, 0, 1),
    "dgcnn_std_bf16": ("dgcnn", STD, 128, 16, 1, 1),
    "dgcnn_general": ("dgcnn", DGCNN_GENERAL["mixed"], 128, 5, 0, 1),
    # ragged tiles (N = 200: 64-point tiles 3 + 8 rows, 128-point tiles 1 + 72 rows) with every per-cloud kernel dealt to several workgroups per cloud
    # (B this small leaves the chip empty: pn_parts / p3_parts / dg_parts pick up to four parts) -- the split against the ORACLE, not against parts = 1
    "pointnet_std_ragged": ("pointnet", STD, 200, 12, 0, 1),
    "pointnet_std_bf16_ragged": ("pointnet", STD, 200, 24, 1, 1),
    "dgcnn_std_ragged": ("dgcnn", STD, 200, 6, 0, 1),
}


@pytest.mark.parametrize("case", sorted(PINNED_CASES))
def test_gradients_match_autograd_with_pinned_decisions(gpu_required, case):
    """Every training code path once more, with the oracle PINNED to the engine's own decisions (alignnet_debug_train_decisions: yaw
    classes models/tp8.py:296, max-pool winners utils/tf_util.py:350-373, and for dgcnn the neighbour slots models/tp8.py:42 and the
    neighbour table utils/tf_util_dgcnn.py:638-676) instead of re-deciding them in fp64.  Two checks:
      * the decisions themselves: each engine winner must be a maximum of the oracle's own values (fp32: to within 1e-4 of their
        scale -- rounding of the fp32 forward; bf16 convs: 2e-2, the operand rounding) and the neighbour table a k-nearest set in
        fp64 distances -- this is the test of the arg-max / selection kernels, on the fused, hybrid and layer-by-layer paths;
      * the rest, held to the oracle's own floor on the batch: every tensor and the whole gradient within max(5e-4, 3 x the worst of
        four self-distances of the pinned fp64 oracle under one-ulp moves of its inputs) (bf16 convs: max(2e-2, 1.5 x))."""
    backbone, w, N, B, bf16, tail = PINNED_CASES[case]
    pinned_check(case, PINNED_CASES[case], R.synth_pairs(B, N, seed=13, dtype=np.float32))


def pinned_check(case, shape, d):
    """Body of test_gradients_match_autograd_with_pinned_decisions on the batch `d` (tests/test_sampler_clouds_gpu.py runs it on batches as the sampler draws them)."""
    backbone, w, N, B, bf16, tail = shape
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), backbone=backbone, **w)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=13)
    rng = np.random.default_rng(13)
    du = {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    eng.set_option("train_fused_tail", tail)
    eng.set_option("train_matmul_bf16", bf16)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    dec = eng.debug_train_decisions(B, relu=True)   # (+ the sign every relu saw: alignnet_debug_train_relu_mask on the fused, hybrid and layer-by-layer paths)
    round_pin = bool(bf16)   # (every bf16 case of PINNED_CASES runs on fused stages)
    if round_pin:
        dec["round"] = eng.debug_train_rounded(B)     # bf16, fused PointNet stages: the operand roundings pinned too (alignnet_debug_train_rounded)
        with pytest.raises(alignnet3d.EngineError):
            eng._check(eng._lib.alignnet_debug_train_rounded(eng._h, 0, 2, None, 0))   # no such layer
    assert dec["yaw"].shape == (2, B) and dec["yaw"].min() >= 0 and dec["yaw"].max() < 12
    for s_, a in enumerate(dec["pool"]):
        assert a.min() >= 0 and a.max() < N, (s_, a.min(), a.max())
    if backbone == "dgcnn":
        assert dec["knn"].shape == (2, B, N, 20) and all(a.min() >= 0 and a.max() < 20 for a in dec["slot"])
    rep = []
    ep_ref, loss_ref, grads, ema_ref = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], bf16_lift=bool(bf16), pinned=dec, report=rep)
    gap_bar = 2e-2 if bf16 else 1e-4
    kinds = {}
    for what, gap, scale, differ, total in rep[0]:
        k = what.split(":")[0]
        kinds[k] = max(kinds.get(k, 0.0), gap / max(scale, 1.0))
    print(case, "pinned: worst decision gap / scale", kinds, "not the oracle's own first maximum:", sum(r[3] for r in rep[0]), "of", sum(r[4] for r in rep[0]))
    assert set(kinds) == ({"yaw", "pool", "relu", "losscls"} if backbone == "pointnet" else {"yaw", "pool", "slot", "knn", "relu", "losscls"}) | ({"round", "roundtail"} if round_pin else set())
    if round_pin:   # every rounded value a bf16 neighbour of the oracle's (a handful of h2 rows further: oracle/alignnet_torch.py _round_bf16_st); the other gaps are then fp32-sized
        assert kinds.pop("round") <= 64.0 and kinds.pop("roundtail") <= 1e-4, kinds
        gap_bar = 1e-3
    assert all(g <= gap_bar for g in kinds.values()), kinds
    n_relu, d_relu = sum(r[4] for r in rep[0] if r[0].startswith("relu")), sum(r[3] for r in rep[0] if r[0].startswith("relu"))
    assert d_relu <= (1e-3 if bf16 else 1e-5) * n_relu + 4, (d_relu, n_relu)   # signs that differ from the oracle's own: a handful, each with |bn(z)| within gap_bar of zero
    # the continuous rest against the oracle's own floor (tests/test_fullsize_gpu.py::_oracle_noise_floor has the story: the relu signs
    # within one rounding of zero): the pinned oracle four more times with its inputs moved by one ulp; the engine must be within
    # max(floor, 3 x the worst of those self-distances)
    from tests.test_fullsize_gpu import _grad_compare, _oracle_noise_floor
    ge = {n: eng.get_gradient(n).astype(np.float64) for n in R.trainable_names(spec)}
    _, relf, cos, rl2, _ = _grad_compare(ge.__getitem__, spec, grads)
    decay = eng.state()["bn_decay"]
    srl2, stens, spred = _oracle_noise_floor(lambda dd: _oracle(cfg, P32, dd, du, decay, bf16_lift=bool(bf16), pinned=dec), d, spec, grads, ep_ref, 4)
    pred = max(float(np.abs(res[k] - ep_ref[k]).max()) for k in ep_ref)
    floor, kc = (2e-2, 1.5) if bf16 else (5e-4 if B >= 8 else 3e-3, 3.0)   # (B < 8: five-row batch statistics in the heads; the free tests allow 1e-2 there)
    if round_pin:
        floor = 1.5e-2   # (roundings pinned: the oracle's self-distance is ~1e-6 and the bar is this floor -- the backward's own bf16 roundings; measured 5e-3 at full size)
    bar_t, bar_l2, bar_p = max(floor, kc * stens), max(floor, kc * srl2), max((2e-4 if round_pin else 2e-2) if bf16 else 1e-4, kc * spred)   # (roundings pinned: the bf16 forward at fp32 level)
    print(case, "pinned: engine vs oracle: predictions %.2e, relative L2 %.2e, worst tensor %.2e (%s) | oracle under one-ulp input moves (worst of 4): predictions %.2e, "
          "relative L2 %.2e, worst tensor %.2e" % (pred, rl2, max(relf.values()), max(relf, key=relf.get), spred, srl2, stens))
    assert pred <= bar_p, (pred, bar_p)
    # (bf16 convs: the loss follows the predictions, which the rounded oracle itself moves by `spred` -- 7e-2 on the five-pair dgcnn case -- under one-ulp moves)
    assert abs(res["loss"] - loss_ref) <= (max(5e-3, 0.2 * spred) if bf16 else 1e-5) * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    assert rl2 <= bar_l2, (rl2, bar_l2)
    bad = {n: e for n, e in relf.items() if e > bar_t}
    assert not bad, (bar_t, bad)
    with pytest.raises(alignnet3d.EngineError):
        eng._check(eng._lib.alignnet_debug_train_decisions(eng._h, 1, 0, dec["yaw"].ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_int32)), 3))   # wrong count
    # the relu-mask hook: shapes as documented (include/alignnet_hip.h), and its refusals
    import ctypes as C
    o = cfg["model"]["options"]
    convs = [list(o["s1transformer"][0]), list(o["s2transformer"][0]), list(o["embedding"])]
    scopes = ["transformer1/embedding", "transformer2/embedding", "embedding"]
    for s_ in range(3):
        nl = len(convs[s_])
        for l, c in enumerate(convs[s_]):
            rows = B if l == nl - 1 else (B * N if (backbone != "dgcnn" or l == nl - 2) else B * N * 20)
            for t in range(2):
                m = dec["relu"][f"{t}:{scopes[s_]}/conv{l + 1}"]
                assert m.shape == (rows, c) and m.dtype == bool and (l == nl - 1 or 0 < m.mean() < 1), (s_, l, t, m.shape, m.mean())
    assert dec["relu"]["p:fc1"].shape == (B, 64) and dec["relu"]["0:transformer1/mlp/fc2"].shape == (B, 32)
    buf = np.empty(8, np.uint8)
    for kind, stage, layer in ((0, 3, 0), (0, 0, 99), (1, 0, 2), (7, 0, 0), (0, 0, 0)):   # bad stage, bad conv layer, no such hidden head layer, bad kind, wrong count
        with pytest.raises(alignnet3d.EngineError):
            eng._check(eng._lib.alignnet_debug_train_relu_mask(eng._h, kind, stage, layer, buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size))
    eng.close()
