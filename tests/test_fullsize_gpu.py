"""GPU: BASELINE.json's full sizes.  Inference (configs[1]: SynthCars widths, B = 256, N = 1024): every pair against the fp64 oracle
plus size-independent properties of the path.  Training (configs[2], [3]'s global batch, [4]'s N): every gradient against fp64
autograd PINNED to the engine's decisions (max-pool winners, yaw classes, neighbour slots, kNN graph) AND to the sign every relu saw,
where the step is a smooth function of its inputs and the bars are sharp: relative L2 1e-4 on the whole gradient, 1e-3 per tensor."""
import numpy as np
import pytest

import alignnet3d
from oracle import alignnet_ref as R
from tests.helpers import oracle_params, compare_forward, compare_forward_all

pytestmark = pytest.mark.gpu
B, N = 256, 1024


@pytest.fixture(scope="module")
def setup():
    cfg = alignnet3d.default_model_config()
    spec, P32 = oracle_params(cfg)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    d = R.synth_pairs(B, N, seed=4321, dtype=np.float32)
    base = eng.forward(d["pcs1"], d["pcs2"])
    yield cfg, spec, P32, eng, d, base
    eng.close()


def _stable(base, nb, eps=1e-3):
    def margin(lg):
        s = np.sort(lg[:, :nb], axis=1)
        return s[:, -1] - s[:, -2]
    return (margin(base["pred_pc1angle_logits"]) > eps) & (margin(base["pred_pc2angle_logits"]) > eps)


def test_finite_and_deterministic(gpu_required, setup):
    cfg, spec, P32, eng, d, base = setup
    again = eng.forward(d["pcs1"], d["pcs2"])
    for k, v in base.items():
        assert np.all(np.isfinite(v)), k
        np.testing.assert_array_equal(v, again[k])


def test_point_permutation_invariance(gpu_required, setup):
    """max-pool and mean are order-free (models/tp8.py:58,104); only the fp32 centroid summation order changes."""
    cfg, spec, P32, eng, d, base = setup
    perm = np.random.default_rng(0).permutation(N)
    out = eng.forward(d["pcs1"][:, perm], d["pcs2"][:, perm])
    ok = _stable(base, spec.num_bins)
    for k in base:
        sel = ok if k in ("pred_translations", "pred_remaining_angle_logits") else slice(None)
        np.testing.assert_allclose(out[k][sel], base[k][sel], rtol=1e-4, atol=1e-4, err_msg=k)


def test_translation_equivariance(gpu_required, setup):
    """Shifting both clouds by t shifts every predicted centre by t and leaves translation / logits unchanged."""
    cfg, spec, P32, eng, d, base = setup
    t = np.array([1.5, -2.25, 0.5], np.float32)
    out = eng.forward(d["pcs1"] + t, d["pcs2"] + t)
    ok = _stable(base, spec.num_bins)
    for k in ("pred_s1_pc1centers", "pred_s1_pc2centers", "pred_s2_pc1centers", "pred_s2_pc2centers"):
        np.testing.assert_allclose(out[k], base[k] + t, rtol=0, atol=2e-4, err_msg=k)
    for k in ("pred_pc1angle_logits", "pred_pc2angle_logits"):
        np.testing.assert_allclose(out[k], base[k], rtol=1e-4, atol=1e-4, err_msg=k)
    np.testing.assert_allclose(out["pred_translations"][ok], base["pred_translations"][ok], rtol=0, atol=3e-4)


def test_pairs_are_independent_and_towers_swap(gpu_required, setup):
    """Eval-mode pairs do not interact (any split of the batch gives the same rows); feeding (pcs2, pcs1) through
    towers with swapped BN sets swaps the per-tower outputs."""
    cfg, spec, P32, eng, d, base = setup
    part = eng.forward(d["pcs1"][100:137], d["pcs2"][100:137])
    for k in base:
        np.testing.assert_array_equal(part[k], base[k][100:137])
    swapped = {}
    for k, v in P32.items():
        k2 = k.replace("siamese_1/", "@@/").replace("siamese/", "siamese_1/").replace("@@/", "siamese/") if "/bn/" in k else k
        swapped[k2] = v
    eng2 = alignnet3d.Engine(cfg)
    eng2.set_variables(swapped)
    out = eng2.forward(d["pcs2"], d["pcs1"])
    eng2.close()
    np.testing.assert_array_equal(out["pred_s2_pc1centers"], base["pred_s2_pc2centers"])
    np.testing.assert_array_equal(out["pred_pc2angle_logits"], base["pred_pc1angle_logits"])


def test_every_pair_against_the_fp64_oracle(gpu_required, setup):
    """configs[1] at its own size: ALL 256 pairs of the batch against the fp64 NumPy oracle (eval-mode pairs are independent, so the
    oracle walks the batch in chunks of 32 to bound its [rows, 1024] activations), north_star's 1e-4 bar on every output of every
    pair: once with the stage-3 outputs of pairs whose yaw decode sits within 1e-3 of a tie counted and left out (compare_forward), and once
    with nothing left out, the oracle pinned to the engine's yaw class on the pairs where the two differ (compare_forward_all)."""
    import time
    cfg, spec, P32, eng, d, base = setup
    P64 = {k: v.astype(np.float64) for k, v in P32.items()}
    t0 = time.time()
    worst_all, unstable_all, worst_every, pinned_all = {}, 0, {}, 0
    for lo in range(0, B, 32):
        sl = slice(lo, lo + 32)
        ref, _, aux = R.get_model(P64, spec, d["pcs1"][sl].astype(np.float64), d["pcs2"][sl].astype(np.float64))
        worst, unstable = compare_forward({k: v[sl] for k, v in base.items()}, ref, spec.num_bins)
        unstable_all += unstable
        for k, v in worst.items():
            worst_all[k] = max(worst_all.get(k, 0.0), v)
        # no pair left out: the oracle re-run pinned to the engine's yaw class on the pairs where the two differ (tests/helpers.py compare_forward_all)
        worst, pinned, left_out = compare_forward_all({k: v[sl] for k, v in base.items()}, ref, aux, P64, spec, d["pcs1"][sl], d["pcs2"][sl])
        assert left_out == []
        pinned_all += pinned
        for k, v in worst.items():
            worst_every[k] = max(worst_every.get(k, 0.0), v)
    print("full size, ALL %d pairs with nothing left out: %d pinned to the engine's yaw class, worst abs err %.3e (%s)"
          % (B, pinned_all, max(worst_every.values()), max(worst_every, key=worst_every.get)))
    print("full size, all %d pairs vs fp64 oracle: worst abs err %.3e (%s), unstable %d, oracle time %.1f s"
          % (B, max(worst_all.values()), max(worst_all, key=worst_all.get), unstable_all, time.time() - t0))
    assert unstable_all <= B // 16


def test_training_reduces_loss_at_full_size(gpu_required):
    """A few Adam steps on one fixed batch of 256 pairs must lower the reference loss (train.py:368 semantics)."""
    cfg = alignnet3d.default_model_config()
    cfg["training"]["batch_size"] = B
    cfg["data"]["ntrain"] = 100 * B
    eng = alignnet3d.Engine(cfg, seed=3)
    d = R.synth_pairs(B, N, seed=7, dtype=np.float32)
    u = [np.full((B, 256), 0.9, np.float32)] * 5   # dropout off (keep + u >= 1) so that the loss is comparable step to step
    losses = [eng.train_step(d["pcs1"], d["pcs2"], d, u)["loss"] for _ in range(25)]
    print("losses", [round(x, 4) for x in losses])
    assert np.all(np.isfinite(losses)) and min(losses[-5:]) < 0.85 * losses[0]
    assert eng.state()["step"] == 25
    eng.close()


def test_bf16_training_learns_like_fp32(gpu_required):
    """BASELINE.json configs[2]: with the 128 -> C3 lifts on bf16 MFMA the network must still learn.  120 Adam steps on fresh
    synthetic batches (64 pairs x 512 points, SynthCars widths) from the same initialisation and the same batch sequence:
    both runs must cut the training loss by >= 30 % (mean of the first vs the last 10 steps), end within 15 % of each other,
    and give finite eval-mode predictions whose held-out translation errors are within a factor of two of each other (the two
    trajectories diverge step by step, so only the trend is comparable)."""
    Bs, Ns, steps = 64, 512, 120
    cfg = alignnet3d.default_model_config()
    cfg["model"]["num_points"] = Ns
    cfg["training"]["batch_size"] = Bs
    cfg["data"]["ntrain"] = 50 * Bs
    held = R.synth_pairs(Bs, Ns, seed=999, dtype=np.float32)
    final = {}
    for mode in (0, 1):
        eng = alignnet3d.Engine(cfg, seed=3)
        eng.set_option("train_matmul_bf16", mode)
        losses = []
        for k in range(steps):
            d = R.synth_pairs(Bs, Ns, seed=1000 + k, dtype=np.float32)
            losses.append(eng.train_step(d["pcs1"], d["pcs2"], d)["loss"])
        pred = eng.forward(held["pcs1"], held["pcs2"])["pred_translations"]
        err = float(np.linalg.norm(pred - held["translations"], axis=1).mean())
        final[mode] = (float(np.mean(losses[:10])), float(np.mean(losses[-10:])), err)
        eng.close()
        assert np.all(np.isfinite(losses)) and np.isfinite(pred).all()
    print("mean loss first / last 10 steps, held-out translation error: fp32", final[0], "bf16", final[1])
    for mode in (0, 1):
        assert final[mode][1] < 0.7 * final[mode][0], final
    assert abs(final[1][1] - final[0][1]) < 0.15 * final[0][1], final
    # held-out error after only 120 steps is a noisy statistic of a chaotic trajectory: the fp32 run alone moved from 0.62 to 0.39 when
    # the optimiser's constants changed in the 7th digit (round 2).  Bound: within a factor of two of each other.
    assert final[1][2] < 2.0 * final[0][2] + 0.05 and final[0][2] < 2.0 * final[1][2] + 0.05, final


def test_bf16_converges_like_fp32(gpu_required):
    """BASELINE.json configs[2] trains: a shortened run of tools/convergence_ab.py (the committed full A/B is profiles/r05_convergence.json:
    3000 steps, three seeds each) -- 1500 steps of 256 pairs x 1024 points from a fixed 2048-example dataset through the device sampler,
    the reference's loop and schedules (train.py:335-383), held-out eval-mode metrics taken as evaluation.py:128-289 takes them.
    bf16's final held-out translation and angle errors (mean over its seeds) must lie within the fp32 seeds' spread + 10 %, both must
    have learnt (held-out errors far below the untrained net's), and every loss and prediction must be finite."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import convergence_ab as CA
    res = CA.run_ab(steps=1500, seeds=3, every=750, n_train=2048, n_held=512)
    s = res["summary"]
    print("convergence A/B (1500 steps):", s)
    for r in res["runs"]:
        assert r["finite_losses"] and all(c["finite"] for c in r["curve"]), (r["dtype"], r["seed"])
        first, last = r["curve"][0], r["curve"][-1]
        assert last["train_loss_mean"] < first["train_loss_mean"], (r["dtype"], r["seed"], first["train_loss_mean"], last["train_loss_mean"])
    for key, slack in (("mean_dist_translation", 0.003), ("mean_dist_angle", 0.5)):   # (+ 3 mm / half a degree: the spread of three seeds is itself a noisy statistic)
        assert s[key]["bf16"]["mean"] <= 1.10 * s[key]["f32"]["max"] + slack, (key, s[key])
    assert s["mean_dist_translation"]["f32"]["mean"] < 0.25 and s["mean_dist_translation"]["bf16"]["mean"] < 0.25, s   # (translations are U(0, 1) m long: an untrained net sits at ~0.5 m)


def test_dgcnn_training_learns(gpu_required):
    """The DGCNN branch (tp8.py:30-46) trains end to end: 120 Adam steps on fresh synthetic batches (32 pairs x 256 points,
    SynthCars widths, k = 20 graph rebuilt every step) cut the training loss by >= 25 % (mean of the first vs the last 10
    steps), and the eval-mode forward afterwards (EMA statistics, same kNN kernels) is finite."""
    Bs, Ns, steps = 32, 256, 120
    cfg = alignnet3d.default_model_config()
    cfg["model"]["num_points"] = Ns
    cfg["model"]["backbone"] = "dgcnn"
    cfg["training"]["batch_size"] = Bs
    cfg["data"]["ntrain"] = 50 * Bs
    eng = alignnet3d.Engine(cfg, seed=3)
    losses = []
    for k in range(steps):
        d = R.synth_pairs(Bs, Ns, seed=2000 + k, dtype=np.float32)
        losses.append(eng.train_step(d["pcs1"], d["pcs2"], d)["loss"])
    held = R.synth_pairs(Bs, Ns, seed=998, dtype=np.float32)
    pred = eng.forward(held["pcs1"], held["pcs2"])["pred_translations"]
    eng.close()
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print("dgcnn mean loss first / last 10 steps:", first, last)
    assert np.all(np.isfinite(losses)) and np.isfinite(pred).all()
    assert last < 0.75 * first, (first, last)


def _train_setup(backbone="pointnet", Bt=B, Nt=N, seed=5):
    cfg = alignnet3d.default_model_config()
    cfg["model"]["num_points"] = Nt
    cfg["model"]["backbone"] = backbone
    cfg["training"]["batch_size"] = Bt
    spec, P32 = oracle_params(cfg, seed=seed)
    d = R.synth_pairs(Bt, Nt, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed)
    du = {k: rng.uniform(size=(Bt, 256)).astype(np.float32) for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")}
    return cfg, spec, P32, d, du


def _grad_compare(get, spec, grads):
    """gradient `get(name)` vs the oracle gradient `grads`: ({tensor: max error / the tensor's own largest reference entry}, the same with the
    denominator floored at 2 % of the whole gradient's largest entry (tensors whose exact value is ~0 do not dominate), cosine,
    relative L2 of the whole gradient, scale)"""
    gscale = max(float(np.abs(v).max()) for v in grads.values())
    bn_bias = {(f"siamese/{L.name}" if L.siamese else L.name) + "/biases" for L in R.layer_table(spec) if L.bn}
    rel, relf = {}, {}
    names = [n for n in R.trainable_names(spec) if n not in bn_bias]
    for name in R.trainable_names(spec):
        g = np.asarray(get(name), np.float64)
        ref = np.asarray(grads[name], np.float64).reshape(g.shape)
        if name in bn_bias:
            assert np.abs(ref).max() < 1e-9 * gscale, name
            continue
        err, top = float(np.abs(g - ref).max()), float(np.abs(ref).max())
        if top > 1e-6 * gscale:
            rel[name] = err / top
        relf[name] = err / max(top, 2e-2 * gscale)
    gv = np.concatenate([np.asarray(get(n), np.float64).ravel() for n in names])
    rv = np.concatenate([np.asarray(grads[n], np.float64).ravel() for n in names])
    cos = float(gv @ rv / (np.linalg.norm(gv) * np.linalg.norm(rv)))
    rl2 = float(np.linalg.norm(gv - rv) / np.linalg.norm(rv))
    return rel, relf, cos, rl2, gscale


def _pin_gaps(report, tag):
    """The oracle's check of every pinned decision: worst (true extreme - value at the engine's winner) / scale per kind, and how many of
    the engine's winners are not the oracle's own first maximum (exact ties -- relu-dead channels, where every point is a maximum -- and
    re-decided near-ties)."""
    out = {}
    for what, gap, scale, differ, total in report:
        k = what.split(":")[0]
        g, dn, tn = out.get(k, (0.0, 0, 0))
        out[k] = (max(g, gap / max(scale, 1.0)), dn + differ, tn + total)
    print(tag, "pinned decisions: " + ", ".join("%s worst gap %.2e of scale, %d of %d differ from the oracle's own choice" % (k, g, dn, tn) for k, (g, dn, tn) in sorted(out.items())))
    return out


def _one_rounding(d, seed=99):
    """the batch with every point coordinate moved to a NEIGHBOURING fp32 value (+- 1 ulp, random sign): what an fp32 evaluation cannot
    tell apart from the batch itself"""
    rng = np.random.default_rng(seed)
    out = dict(d)
    for k in ("pcs1", "pcs2"):
        x = np.asarray(d[k], np.float32)
        out[k] = np.nextafter(x, x + np.where(rng.random(x.shape) < 0.5, -1, 1).astype(np.float32)).astype(np.float32)
    return out


def _oracle_noise_floor(oracle, d, spec, grads, ep_ref, trials):
    """How far the PINNED fp64 oracle moves from itself when its inputs move by one ulp, worst of `trials` draws: (relative L2 of the
    whole gradient, worst tensor, predictions).  What is left undecided after the pins are the SIGNS of the relu pre-activations
    (utils/tf_util.py:152,339: ~10^6 .. 10^8 per step); the handful that sit within one rounding of zero flip between any two
    evaluations, and a flip on a row that wins many max-pool channels re-routes ~1 % of a weight column's gradient.  Measured at
    16 x 256 points: the draws give 3e-5 .. 1e-2 (one seed) and 3e-5 .. 5e-2 (another) in QUANTISED steps -- the same flip recurring --
    so one draw says little and the worst of several is the floor."""
    worst = [0.0, 0.0, 0.0]
    for t in range(trials):
        ep2, _, g2, _ = oracle(_one_rounding(d, 99 + t))
        _, sens_f, _, srl2, _ = _grad_compare(lambda n: g2[n], spec, grads)
        worst = [max(worst[0], srl2), max(worst[1], max(sens_f.values())), max(worst[2], max(float(np.abs(ep2[k] - ep_ref[k]).max()) for k in ep_ref))]
    return worst


def _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel, pred_tol, loss_tol, ema_tol, rl2_bar=1e-4, tensor_bar=1e-3, cos_bar=None,
                                  free=None, bf16=False, gap_bar=1e-4, relu_gap_bar=1e-4, relu_differ_bar=1e-5, tag="full size", round_pin=False, round_gap_bar=1.0):
    """Train-mode forward (batch statistics over all 2 x B x N points, EMA), loss and every parameter gradient against the torch-autograd
    oracle in fp64 (backbones recomputed in the backward: oracle/alignnet_torch.py `checkpoint`), FULLY PINNED to the engine's step:

    (1) the DECISIONS (Engine.debug_train_decisions: 0.9 M max-pool winners utils/tf_util.py:350-373 and 512 yaw classes models/tp8.py:296
        at 256 x 1024; neighbour slots and the kNN table for dgcnn): the oracle gathers at them after checking that each is a maximum of its
        own values to within `gap_bar` of their scale (measured 1e-6) -- the test of the arg-max / selection kernels; and the class
        tf_angle2class (models/tp8.py:193-199) put every target angle of the loss into -- 2 x 65,536 of them in the pair term's [B, B] target
        (:327): the residual label is a sawtooth in the angle, one entry within a rounding of a class boundary lands on the other tooth in
        another evaluation, and that one flip moved the whole gradient by 4e-4 on the `same` batch of seed 1 (profiles/r06_relu_pin_seeds.log);
        checked: differing entries within `gap_bar` classes of the boundary;
    (2) the SIGN every relu saw (alignnet_debug_train_relu_mask: 6e8 bits at 256 x 1024, utils/tf_util.py:167-168,345-346): the oracle
        evaluates y = bn(z) * mask after checking that wherever the mask disagrees with its own sign |bn(z)| <= `relu_gap_bar` of the layer's
        scale and that at most `relu_differ_bar` of the signs disagree (measured: ~600 of 6e8, |bn(z)| 4e-6 of scale) -- the test of the BatchNorm /
        relu arithmetic of every pass;
    (3) with (1) and (2) fixed the step is a SMOOTH function of its inputs and the comparison is sharp: whole-gradient relative L2 <= 1e-4,
        every tensor within 1e-3 of max(its largest entry, 2 % of the gradient's largest).  Round 5 stopped at (1) and found the distance
        unchanged at 1e-2: the undecided rest were the relu signs within a rounding of zero (~600 flips re-route per cents of a weight column's
        gradient).  Pinned, a plain fp32 evaluation of the graph (torch, tools/relu_pin_diag.py) sits 1e-5 .. 3e-5 from the fp64 one, and so does the engine.
        (Round 6's first runs read 4.4e-4 on the `varied` batch and 4.3e-4 on `same`, seed 1: one entry each of the loss's angle-class matrix on the other
        side of its boundary -- item (1); DESIGN.md 2 has the wrong turn that preceded that finding.)
    `free`: additionally the oracle deciding everything for itself, held to the loose fixed bars given (cos, rl2, per tensor) -- one case keeps
    it so that the unpinned agreement stays on record; its floor is the re-decided signs, not this implementation."""
    from tests import test_train_gpu as TT
    us = [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")]
    Bt = d["pcs1"].shape[0]
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    eng.set_option("train_matmul_bf16", int(bf16))
    decay = eng.state()["bn_decay"]
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
    assert eng.get_option("last_train_kernel") == expect_kernel
    decisions = eng.debug_train_decisions(Bt, relu=True)
    if bf16 and round_pin:
        decisions["round"] = eng.debug_train_rounded(Bt)   # the bf16-rounded h1 / h2 the step's MFMA convs multiplied
    ge = {n: eng.get_gradient(n).astype(np.float64) for n in R.trainable_names(spec)}
    bn_bias = {(f"siamese/{L.name}" if L.siamese else L.name) + "/biases" for L in R.layer_table(spec) if L.bn}
    assert all(np.abs(ge[n]).max() == 0.0 for n in bn_bias)
    ema_got = None
    failures = []
    if bf16:
        tag += " bf16"
    for mode in (("free",) if free else ()) + ("pinned",):
        rep = []
        ep_ref, loss_ref, grads, ema_ref = TT._oracle(cfg, P32, d, du, decay, bf16_lift=bf16, checkpoint=True, pinned=decisions if mode == "pinned" else None, report=rep)
        if ema_got is None:
            ema_got = {k: eng.get_variable(k) for k in ema_ref}
        worst_pred = max(float(np.abs(res[k] - ep_ref[k]).max()) for k in ep_ref)
        worst_ema = max(float(np.abs(ema_got[k] - v).max()) for k, v in ema_ref.items())
        ema_fail = [k for k, v in ema_ref.items() if not np.allclose(ema_got[k], v, rtol=ema_tol, atol=0.1 * ema_tol)]
        rel, relf, cos, rl2, gscale = _grad_compare(ge.__getitem__, spec, grads)
        print("%s (%s): loss %.6f (oracle %.6f), worst prediction err %.2e, worst EMA err %.2e, whole gradient: cosine %.10f, relative L2 error %.2e, "
              "worst tensors (error / max(own largest, 2 %% of the gradient's)) %s" % (tag, mode, res["loss"], loss_ref, worst_pred, worst_ema, cos, rl2,
                                                                                    [(k, float("%.2g" % v)) for k, v in sorted(relf.items(), key=lambda kv: -kv[1])[:4]]))
        if worst_pred > pred_tol: failures.append((mode + " predictions", worst_pred))
        if abs(res["loss"] - loss_ref) > loss_tol * max(1.0, abs(loss_ref)): failures.append((mode + " loss", res["loss"], loss_ref))
        if ema_fail: failures.append((mode + " EMA", ema_fail[:4]))
        if mode == "free":
            if cos < free["cos"] or rl2 > free["rl2"]: failures.append(("free whole gradient", cos, rl2))
            bad = {n: e for n, e in rel.items() if e > free["tensor"] and relf[n] > 1e-3}
            if bad: failures.append(("free tensors", bad))
            continue
        gaps = _pin_gaps(rep[0], tag + ":")
        bar_of = {"relu": relu_gap_bar, "round": round_gap_bar, "roundtail": 1e-5}   # (roundtail: the FRACTION of rounded values further than 1.5 bf16 steps from the oracle's)
        if any(g > bar_of.get(k, gap_bar) for k, (g, _, _) in gaps.items()): failures.append(("a pinned decision / sign is not the oracle's to within rounding", gaps))
        if "relu" not in gaps or gaps["relu"][1] > relu_differ_bar * gaps["relu"][2]: failures.append(("relu signs", gaps.get("relu")))
        if rl2 > rl2_bar: failures.append(("pinned whole gradient", rl2, rl2_bar))
        if cos_bar is not None and cos < cos_bar: failures.append(("pinned cosine", cos, cos_bar))
        bad = {n: e for n, e in relf.items() if e > tensor_bar}
        if bad: failures.append(("pinned tensors", tensor_bar, bad))
    eng.close()
    assert not failures, failures


def _varied_setup(backbone="pointnet", Bt=B, Nt=N, seed=5):
    """_train_setup on a batch of differently sized objects (tests/helpers.varied_pairs: real batches hold different objects; with ONE box shape
    every canonicalised cloud looks alike and the heads' batch normalisation divides by sampling noise)"""
    from tests.helpers import varied_pairs
    cfg, spec, P32, _, du = _train_setup(backbone, Bt, Nt, seed)
    return cfg, spec, P32, varied_pairs(Bt, Nt, seed=seed, dtype=np.float32), du


def test_train_fp32_full_size_matches_autograd(gpu_required):
    """BASELINE.json configs[2]'s shape in fp32: SynthCars widths, 256 pairs x 1024 points -- the kernel instantiations with the
    widths compiled in, whole-cloud tile walks, 512 workgroups, the B x B loss terms at B = 256.  Measured pinned: relative L2 2.3e-5
    (a plain torch fp32 evaluation: 2.8e-5).  Also FREE, at the loose bars of the re-decided signs (measured 1.3e-2)."""
    cfg, spec, P32, d, du = _train_setup()
    _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel=1, pred_tol=2.5e-4, loss_tol=1e-5, ema_tol=5e-5,
                                  free={"cos": 0.9995, "rl2": 3e-2, "tensor": 8e-2})


def test_train_fp32_full_size_varied_objects(gpu_required):
    """The same step on 256 differently sized objects: the batch on which round 5's report had the engine at 5.4 x the oracle's own noise.  Fully
    pinned: 7.0e-6 (torch fp32: 1.2e-5); 4.4e-4 before the loss's angle classes were pinned (one of 131 k entries on the other tooth)."""
    cfg, spec, P32, d, du = _varied_setup()
    _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel=1, pred_tol=2.5e-4, loss_tol=1e-5, ema_tol=5e-5, tag="full size, varied objects")


def test_train_bf16_full_size_pinned_to_engine_decisions(gpu_required):
    """configs[2] at its own size (bf16 MFMA convs, 256 differently sized objects x 1024 points) against the rounded-operand oracle pinned to
    the engine's winners, classes, relu signs -- and to the bf16-ROUNDED activations h1 / h2 its MFMA convs multiplied (alignnet_debug_train_rounded:
    every rounding of an operand to bf16 is a decision of its own, 2^-8 of the value, 6e8 of them here; the oracle takes the engine's rounded value
    after checking it is a bf16 neighbour of its own).  With the roundings pinned the bf16 FORWARD is an fp32-level statement: predictions within
    2.9e-5 of the oracle's (6.4e-2 unpinned), loss 2.6e-8, and the fully pinned oracle is smooth (2.5e-7 against itself under one-ulp input moves).
    The gradient then measures the backward's own bf16 storage and operand roundings (dy2 kept as bf16 between passes B2 and B1, the bf16 images of
    Q3 / V2 / Q2, hi + lo split of the sparse rows), which the straight-through oracle does not model: cosine 0.999988, relative L2 4.9e-3, worst
    tensor 8.4e-3 of max(own, 2 %) (round 5, winners only: cosine 0.992, 0.138, 0.249; signs and angle classes too: 0.99995, 1.0e-2).  Bars at about
    twice the measured distance.  That the mode TRAINS is test_bf16_converges_like_fp32's statement."""
    cfg, spec, P32, d, du = _varied_setup()
    _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel=3, pred_tol=2e-4, loss_tol=1e-6, ema_tol=5e-5, rl2_bar=1e-2, tensor_bar=2e-2, cos_bar=0.99995,
                                  bf16=True, gap_bar=1e-4, relu_gap_bar=1e-3, relu_differ_bar=1e-5, round_pin=True, round_gap_bar=64.0, tag="full size, varied objects")


@pytest.mark.parametrize("bf16", [0, 1])
def test_train_reference_shipped_shape_matches_autograd(gpu_required, bf16):
    """The shape the reference's own config files train at (configs/*.json: batch_size 128, num_points 512; every one but default.json): 256 clouds do
    not fill the chip's 512 two-per-CU workgroup slots, so phase 2 / the first-layer Gram and passes B2, B1 run with TWO workgroups per cloud (alignnet_train.hip
    pn_parts; phase 3, one workgroup per CU, stays whole) -- the split at scale, against the fully pinned fp64 oracle on 128 differently sized objects, at the
    bars of the 256 x 1024 tests."""
    cfg, spec, P32, d, du = _varied_setup(Bt=128, Nt=512, seed=21)
    if bf16:
        _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel=3, pred_tol=2e-4, loss_tol=1e-6, ema_tol=5e-5, rl2_bar=1e-2, tensor_bar=2e-2, cos_bar=0.99995,
                                      bf16=True, gap_bar=1e-4, relu_gap_bar=1e-3, relu_differ_bar=1e-5, round_pin=True, round_gap_bar=64.0, tag="128 x 512, varied objects")
    else:
        _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel=1, pred_tol=2.5e-4, loss_tol=1e-5, ema_tol=5e-5, tag="128 x 512, varied objects")


def test_train_dgcnn_n1024_matches_autograd(gpu_required):
    """DGCNN training at N = 1024 (the kNN kernel's 16-slot instantiation at its limit, 16 tiles per cloud, 20 neighbour slots,
    SynthCars widths -> dg_train_fwd<64> / dg_train_bwd_edge<64, 128>): B = 8 differently sized objects keep the [B*N*k, C] autograd
    oracle in memory.  Measured pinned: 1.9e-5 (torch fp32 2.5e-5)."""
    cfg, spec, P32, d, du = _varied_setup("dgcnn", Bt=8, Nt=1024, seed=7)
    _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel=5, pred_tol=5e-4, loss_tol=1e-5, ema_tol=2e-4, tag="dgcnn N=1024")


def test_train_b2048_matches_autograd(gpu_required):
    """BASELINE.json configs[3]'s arithmetic on ONE GPU: the global batch of 2048 pairs (KITTITrackletsCarsPersonsHard: SynthCars
    widths) in a single step -- the [B, B] loss terms of models/tp8.py:279,327 at 4 M entries, the whole-batch tf.cond (:288), the
    4096-row head BatchNorms, 4096 workgroups per backbone launch.  N = 128 keeps the fp64 autograd oracle at the cost of the
    256 x 1024 test (the same 524 k points).  Measured pinned: 1.1e-5 (7.1e-5 before the 2 x 4 M angle classes of the pair term were pinned)."""
    cfg, spec, P32, d, du = _varied_setup(Bt=2048, Nt=128, seed=11)
    _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel=1, pred_tol=3e-4, loss_tol=1e-5, ema_tol=2e-5, tag="B=2048")


def test_train_dgcnn_n4096_matches_autograd(gpu_required):
    """BASELINE.json configs[4]'s training half at its own N: DGCNN at N = 4096 (knn_kernel<64>, 64 tiles per cloud, SynthCars
    widths -> dg_train_fwd<64> / dg_train_bwd_edge<64, 128>) against fp64 autograd; B = 8 differently sized objects (1.3 M edge rows,
    [2B, N, N] distance matrices in the oracle; with B = 4 the heads' four-row batch statistics put a plain torch fp32 evaluation of the
    pinned graph 1.5e-4 from the fp64 one -- tools/relu_pin_diag.py -- and the engine at 2.2e-4).  The fp32 kNN graph differs from an fp64 one wherever the 20th and 21st neighbour of a
    query are closer than fp32 rounding of the distance expression (dozens of queries per cloud): pinned, the engine's table is checked as
    a k-nearest SET of every query in fp64 distances (gap 1e-6 of the largest k-th distance) and the step is compared on it.  Measured pinned:
    1.4e-5 (torch fp32 1.5e-5) -- the B = 4 `same` batch sat at 4.2e-3 before round 6 folded Gram(h1), accumulated over a cloud's 82 k edge rows in fp32, into fp64 per tile."""
    cfg, spec, P32, d, du = _varied_setup("dgcnn", Bt=8, Nt=4096, seed=9)
    _check_train_against_autograd(cfg, spec, P32, d, du, expect_kernel=5, pred_tol=5e-4, loss_tol=5e-5, ema_tol=5e-4, tag="dgcnn N=4096")


def test_batch_statistics_per_channel_full_size(gpu_required):
    """Every BatchNorm's batch variance, PER CHANNEL, against the fp64 oracle at 256 differently sized objects x 1024 points (a forward-only oracle run:
    the statistics are continuous in the inputs, nothing needs pinning).  A BatchNorm divides by its own channel's deviation, so the error that matters
    is relative to that channel's value (variance) or deviation (mean), not to the layer's largest.  Measured <= 1.8e-6 (round 5's library: 1.9e-6 -- the
    4.4e-4 round 6 first read on this batch was not in any forward statistic but in one entry of the loss's angle-class matrix).  A guard for
    the statistics kernels, which read fp64 totals and evaluate centred forms since round 6."""
    import torch
    from oracle import alignnet_torch as T
    cfg, spec, P32, d, du = _varied_setup()
    # shadows start at ZERO (as TF's do): the updated shadow is then (1 - decay) x the batch value and carries its relative error undiluted
    P32 = {k: (np.zeros_like(v) if k.endswith(("moving_mean", "moving_var")) else v) for k, v in P32.items()}
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    decay = eng.state()["bn_decay"]
    eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in ("s1_0", "s2_0", "s1_1", "s2_1", "rem")])
    tm = T.TorchTp8(spec, T.to_torch({k: v.astype(np.float64) for k, v in P32.items()}))
    with torch.no_grad():
        tm.forward(torch.tensor(d["pcs1"].astype(np.float64)), torch.tensor(d["pcs2"].astype(np.float64)), True, decay,
                   {k: torch.tensor(v.astype(np.float64)) for k, v in du.items()})
    worst = {}
    for k, v in tm.ema_updates.items():
        ref = v.numpy().ravel()
        got = np.asarray(eng.get_variable(k), np.float64).ravel()
        if k.endswith("moving_var"):
            worst[k] = float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)).max())           # variance: relative, per channel
        else:
            var = tm.ema_updates[k.replace("moving_mean", "moving_var")].numpy().ravel() / (1.0 - decay)
            worst[k] = float((np.abs(got - ref) / (1.0 - decay) / np.sqrt(var + 1e-3)).max())      # mean: in units of the channel's deviation (what zhat sees)
    eng.close()
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("batch statistics per channel, worst (variance: relative; mean: in deviations):", [(k, float("%.2g" % e)) for k, e in top])
    assert max(worst.values()) <= 2e-5, top


def test_train_dgcnn_n4096_b512_runs(gpu_required):
    """configs[4] at one GPU's share of the batch (4096 / 8 = 512 pairs, N = 4096): two full training steps (fp32, then bf16
    convs) -- finite loss, the expected kernel instantiations, a parameter update -- and an eval forward afterwards."""
    Bs, Ns = 512, 4096
    cfg = alignnet3d.default_model_config()
    cfg["model"]["num_points"] = Ns
    cfg["model"]["backbone"] = "dgcnn"
    cfg["training"]["batch_size"] = Bs
    eng = alignnet3d.Engine(cfg, seed=3)
    d = R.synth_pairs(Bs, Ns, seed=21, dtype=np.float32)
    w0 = eng.get_variable("siamese/embedding/conv3/weights").copy()
    r0 = eng.train_step(d["pcs1"], d["pcs2"], d)
    assert eng.get_option("last_train_kernel") == 5 and np.isfinite(r0["loss"])
    eng.set_option("train_matmul_bf16", 1)
    r1 = eng.train_step(d["pcs1"], d["pcs2"], d)
    assert eng.get_option("last_train_kernel") == 7 and np.isfinite(r1["loss"])
    w1 = eng.get_variable("siamese/embedding/conv3/weights")
    assert np.isfinite(w1).all() and np.abs(w1 - w0).max() > 0
    out = eng.forward(d["pcs1"][:8], d["pcs2"][:8])
    eng.close()
    assert all(np.isfinite(v).all() for v in out.values())
    print("dgcnn N=4096 B=512: losses", r0["loss"], r1["loss"])
