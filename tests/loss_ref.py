"""References and bars of the loss-kernel tests.  The reference is the oracle: R.get_loss / R.get_angles / R.angle2class (dtype-generic NumPy) for decode,
classes and values, T.TorchTp8.loss (autograd) for the gradient, each evaluated in float64 (the truth) and in float32 (the yardstick: what one honest
float32 evaluation of the same graph loses).  The bars are MEASURED here from the reference alone (bars()), never from the code under test:
  values     u_v = worst |oracle32 - oracle64| / max(1, |oracle64|) over the 17 outputs and all value cases; a result passes at 4 u_v
  gradients  u_g = the same per tensor for float32 against float64 autograd, relative to the tensor's largest reference entry; passes at 4 u_g
(the factor 4: the kernels sum in another order -- float per thread over rows, then double).  1e-4, the bar of the rest of the suite, is the ceiling.
judge() holds every check the GPU test applies to a result; the CPU test feeds it the mutated models of loss_model() and must see each refused."""
import functools

import numpy as np
import torch

from oracle import alignnet_ref as R
from oracle import alignnet_torch as T
from tests import loss_cases as LC

F = np.float32
CEILING = 1e-4
GRAD_KEYS = ("d_s1c", "d_s2c", "d_o2", "d_o3")
MUTATIONS = ("pair_label_column0", "cond_picks_smaller", "towers_lose_s3", "stage3_huber_delta1", "half_bin_shift_dropped", "residual_mean_over_B",
             "last_row_slice_dropped", "class_nb_clamped")


def spec_of(case):
    return R.NetSpec(num_bins=case["nb"], accept_inverted_angle=bool(case["accept_inverted"]), early_stage_factor=case["esf"], angle_factor=case["af"])


def endpoints(case, dt):
    """the end points of models/tp8.py:135-158 from the head outputs, as float32 computes them (s2c = o2[:, :3] + s1c), then cast"""
    B, o2, s1c, o3 = case["B"], case["o2"], case["s1c"], case["o3"]
    s2c = (o2[:, :3] + s1c).astype(F)
    ep = {"pred_s1_pc1centers": s1c[:B], "pred_s1_pc2centers": s1c[B:], "pred_s2_pc1centers": s2c[:B], "pred_s2_pc2centers": s2c[B:],
          "pred_pc1angle_logits": o2[:B, 3:], "pred_pc2angle_logits": o2[B:, 3:],
          "pred_translations": o3[:, :3].astype(dt) + (s2c[B:].astype(dt) - s2c[:B].astype(dt)), "pred_remaining_angle_logits": o3[:, 3:]}
    return {k: np.asarray(v, dt) for k, v in ep.items()}, s2c


def _label_args(case, dt):
    return [np.asarray(case["labels"][k], dt) for k in LC.LABEL_KEYS]


def _all_classes(angle, nb):
    """R.angle2class keeps column 0 of the class matrix (models/tp8.py:199); every entry: one column per entry.  (classes, residuals in label units)"""
    k, res = R.angle2class(angle.reshape(-1, 1), nb)
    return k.reshape(angle.shape), (res / angle.dtype.type(F(np.pi / nb))).reshape(angle.shape)


def oracle_values(case, dt):
    """dict: out [17], theta [2B], pcls [2B], cls = [[2, B], [2, B], [2, B, B]], lab = the residual labels in the same layout, tot [3][2] (both variants'
    totals; variant 1 only with accept_inverted)"""
    spec, nb, B = spec_of(case), case["nb"], case["B"]
    ep, _ = endpoints(case, dt)
    lab = _label_args(case, dt)
    loss, summ = R.get_loss(spec, ep, *lab)
    p1, k1 = R.get_angles(ep["pred_pc1angle_logits"], nb)
    p2, k2 = R.get_angles(ep["pred_pc2angle_logits"], nb)
    a1, a2 = lab[4], lab[5]
    targets = (a1, a2, (a2 - a1) - (p2 - p1))
    logits = (ep["pred_pc1angle_logits"], ep["pred_pc2angle_logits"], ep["pred_remaining_angle_logits"])
    pi = dt(F(np.pi))
    cls, lab_res, tot = [], [], []
    for t in range(3):
        both = [_all_classes(targets[t], nb), _all_classes(targets[t] + pi, nb)]
        cls.append(np.stack([b[0] for b in both]).reshape((2, B) if t < 2 else (2, B, B)).astype(np.int32))
        lab_res.append(np.stack([b[1] for b in both]).reshape(cls[-1].shape))
        tot.append([float(R.angle_loss(logits[t], targets[t] + v * pi, nb)[0]) for v in ((0, 1) if case["accept_inverted"] else (0,))])
    return dict(out=np.array([loss] + list(summ.values()), dt), theta=np.concatenate([p1, p2]), pcls=np.concatenate([k1, k2]).astype(np.int32), cls=cls, lab=lab_res, tot=tot)


def choice_of(tot):
    """tf.cond keeps the LARGER total (models/tp8.py:284-291)"""
    return [0 if (len(t) == 1 or t[0] > t[1]) else 1 for t in tot]


def _torch_leaves(case, tdt):
    B, nb = case["B"], case["nb"]
    _, s2c = endpoints(case, F)
    mk = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=tdt, requires_grad=True)
    leaves = dict(s1c=mk(case["s1c"]), s2c=mk(s2c), lg2=mk(case["o2"][:, 3:]), o3=mk(case["o3"]))
    ep = {"pred_s1_pc1centers": leaves["s1c"][:B], "pred_s1_pc2centers": leaves["s1c"][B:],
          "pred_s2_pc1centers": leaves["s2c"][:B], "pred_s2_pc2centers": leaves["s2c"][B:],
          "pred_pc1angle_logits": leaves["lg2"][:B], "pred_pc2angle_logits": leaves["lg2"][B:],
          "pred_translations": leaves["o3"][:, :3] + (leaves["s2c"][B:] - leaves["s2c"][:B]),   # as TorchTp8.forward builds it
          "pred_remaining_angle_logits": leaves["o3"][:, 3:]}
    lab = [torch.tensor(np.asarray(case["labels"][k], np.float64), dtype=tdt) for k in LC.LABEL_KEYS]
    return leaves, ep, lab


def _grads_of(loss, leaves, case):
    g = torch.autograd.grad(loss, [leaves[k] for k in ("s1c", "s2c", "lg2", "o3")], allow_unused=True)
    g = [np.zeros(tuple(leaves[k].shape)) if x is None else x.detach().numpy().astype(np.float64) for x, k in zip(g, ("s1c", "s2c", "lg2", "o3"))]
    d_o2 = np.zeros((2 * case["B"], 3 + 2 * case["nb"]))
    d_o2[:, 3:] = g[2]
    return dict(d_s1c=g[0], d_s2c=g[1], d_o2=d_o2, d_o3=g[3])


def oracle_grads(case, tdt=torch.float64):
    """autograd of T.TorchTp8.loss; leaves s1c, s2c, the logits of o2, o3 (so d_s2c holds the pred_translations path and d_o2[:, :3] is zero: what the
    loss kernels leave in front of the glue backward).  The decoded yaw classes are pinned to np.argmax's (first maximum)."""
    leaves, ep, lab = _torch_leaves(case, tdt)
    B = case["B"]
    win = np.argmax(case["o2"][:, 3:3 + case["nb"]], axis=1)
    m = T.TorchTp8(spec_of(case), {}, pinned={"yaw": [win[:B], win[B:]]})
    return _grads_of(m.loss(ep, *lab), leaves, case)


@functools.lru_cache(maxsize=None)
def reference(c):
    """everything the tests need of one value case, computed once: the case, the oracle in both precisions, the float64 gradient"""
    case = LC.value_case(c)
    v64, v32 = oracle_values(case, np.float64), oracle_values(case, F)
    g64, g32 = oracle_grads(case, torch.float64), oracle_grads(case, torch.float32)
    return dict(case=case, v64=v64, v32=v32, g64=g64, g32=g32)


def rel_values(out, ref64):
    return float(np.max(np.abs(np.asarray(out, np.float64) - ref64) / np.maximum(1.0, np.abs(ref64))))


def rel_grad(g, g64):
    scale = float(np.abs(g64).max())
    err = float(np.abs(np.asarray(g, np.float64) - g64).max())
    return (err / scale) if scale > 0 else (0.0 if err == 0 else np.inf)


@functools.lru_cache(maxsize=None)
def bars():
    """(u_v, {tensor: u_g}) measured on the oracle alone over all value cases"""
    u_v, u_g = 0.0, {k: 0.0 for k in GRAD_KEYS}
    for c in LC.VALUE_CASES:
        r = reference(c)
        u_v = max(u_v, rel_values(r["v32"]["out"], r["v64"]["out"]))
        for k in GRAD_KEYS:
            u_g[k] = max(u_g[k], rel_grad(r["g32"][k], r["g64"][k]))
    return u_v, u_g


def undecided(c):
    """number of label classes of a value case on which the float32 and the float64 oracle disagree -- or whose residual labels sit on different teeth
    (more than one bin's worth apart; nb = 1 has one class, and its only boundary, the wrap of the shifted angle, shows in the residual alone)"""
    r = reference(c)
    v32, v64 = r["v32"], r["v64"]
    nv = 2 if r["case"]["accept_inverted"] else 1   # (without accept_inverted the classes of label + pi enter nothing)
    return sum(int(((a[:nv] != b[:nv]) | (np.abs(x[:nv] - y[:nv]) > 1.0)).sum()) for a, b, x, y in zip(v32["cls"], v64["cls"], v32["lab"], v64["lab"]))


def judge_classes(cls, ref_cls, nb):
    bad = []
    for t in range(3):
        k = np.asarray(cls[t])
        if k.min() < 0 or k.max() >= nb:
            bad.append("term %d: class outside [0, %d): %d .. %d" % (t, nb, k.min(), k.max()))
        n = int((k != ref_cls[t]).sum())
        if n:
            bad.append("term %d: %d of %d classes differ from the float32 oracle" % (t, n, k.size))
    return bad


def judge(res, c, figures=None):
    """Every check of a result (dict as Engine.debug_loss returns it; "theta" / "pcls" / "s2c" optional) of value case c.  List of failures, empty = passes.
    figures (optional dict) collects the measured worst errors."""
    r = reference(c)
    case, v64, v32 = r["case"], r["v64"], r["v32"]
    u_v, u_g = bars()
    bad = []
    if "pcls" in res:
        if not np.array_equal(res["pcls"], v32["pcls"]):
            bad.append("decoded classes differ")
        dth = float(np.abs(res["theta"].astype(np.float64) - v32["theta"].astype(np.float64)).max())
        if dth > 2 * float(np.spacing(F(np.pi))):
            bad.append("theta off by %.3g" % dth)
        if not np.array_equal(res["s2c"], endpoints(case, F)[1]):
            bad.append("s2c is not o2[:, :3] + s1c bit for bit")
    if "cls" in res:
        bad += judge_classes(res["cls"], v32["cls"], case["nb"])
    ev = rel_values(res["out"], v64["out"])
    if not ev <= min(4 * u_v, CEILING):
        bad.append("values off by %.3g (bar %.3g)" % (ev, min(4 * u_v, CEILING)))
    want = choice_of(v64["tot"])
    for t in range(3):
        if len(v64["tot"][t]) == 2:
            got = int(np.argmin([abs(float(res["out"][8 + 3 * t]) - x) for x in v64["tot"][t]]))
            if got != want[t]:
                bad.append("term %d: variant %d chosen, the float64 oracle chooses %d" % (t, got, want[t]))
    if figures is not None:
        figures["values"] = max(figures.get("values", 0.0), ev)
    if "d_o3" in res:
        for k in GRAD_KEYS:
            eg = rel_grad(res[k], r["g64"][k])
            if figures is not None:
                figures[k] = max(figures.get(k, 0.0), eg)
            if not eg <= min(4 * u_g[k], CEILING):
                bad.append("%s off by %.3g (bar %.3g)" % (k, eg, min(4 * u_g[k], CEILING)))
        if np.any(res["d_o2"][:, :3] != 0):
            bad.append("d_o2[:, :3] is not zero")
        if case["af"] == 0 and (np.any(res["d_o2"] != 0) or np.any(res["d_o3"][:, 3:] != 0)):
            bad.append("angle_factor 0: a logit gradient is not exactly zero")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The loss as the KERNELS state it, with one switch per wrong kernel the tests must refuse (tests/test_loss_cpu.py).  float32 NumPy for the class
# rule (what the kernels' angle2class computes: exact fmod, then rounded float32 steps), torch for values and gradient.
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _fmod_floor(x, y):
    r = np.fmod(x, y)
    return np.where((r != 0) & (r < 0), r + y, r).astype(x.dtype)


def kernel_class_rule(angle, nb, rule="wrap"):
    """float32 restatement of the kernels' angle2class: (class, residual, sh).  rule: "wrap" (class nb is class 0, residual as computed), "clamp" (class
    nb - 1, residual as computed: the behaviour before the rule), "raw" (class nb stays), "noshift" (half-bin shift dropped)."""
    angle = np.asarray(angle, F)
    apc = LC.TWOPI / F(nb)
    a = _fmod_floor(angle, LC.TWOPI)
    sh = a if rule == "noshift" else _fmod_floor((a + apc * F(0.5)).astype(F), LC.TWOPI)
    c = (sh / apc).astype(np.int32)
    res = (sh - (c.astype(F) * apc + apc * F(0.5))).astype(F)
    if rule in ("wrap", "noshift"):
        c = np.where(c >= nb, c - nb, c)
    elif rule == "clamp":
        c = np.minimum(c, nb - 1)
    return c.astype(np.int32), res, sh


def model_classes(case, theta, mutation=None):
    """the classes of all three terms as dbg_angle_class_kernel lays them out, from float32 theta [2B]"""
    B, nb = case["B"], case["nb"]
    rule = {"class_nb_clamped": "clamp", "half_bin_shift_dropped": "noshift"}.get(mutation, "wrap")
    a1, a2 = case["labels"]["pc1_angles"][:, 0], case["labels"]["pc2_angles"][:, 0]
    dth = (theta[B:] - theta[:B]).astype(F)
    if mutation == "pair_label_column0":
        dth = np.full(B, dth[0], F)
    pair = ((a2 - a1).astype(F)[:, None] - dth[None, :]).astype(F)
    pi = F(np.pi)
    return [np.stack([kernel_class_rule(t, nb, rule)[0], kernel_class_rule((t + pi).astype(F), nb, rule)[0]]) for t in (a1, a2, pair)]


def loss_model(case, mutation=None, tdt=torch.float64):
    """dict like Engine.debug_loss's (out, cls, gradients), in float64 torch with the classes of the float32 rule."""
    B, nb, ai, esf, af = case["B"], case["nb"], case["accept_inverted"], case["esf"], case["af"]
    leaves, ep, lab = _torch_leaves(case, tdt)
    tr, _, c1, c2, a1, a2 = lab
    theta32 = np.concatenate([R.get_angles(case["o2"][:B, 3:], nb)[0], R.get_angles(case["o2"][B:, 3:], nb)[0]]).astype(F)
    cls = model_classes(case, theta32, mutation)
    twopi, pi = float(LC.TWOPI), float(F(np.pi))
    apc, pinb = twopi / nb, float(F(np.pi / nb))
    hub = lambda e, d: torch.nn.functional.huber_loss(e, torch.zeros_like(e), delta=d)

    def decode(lg):
        win = torch.as_tensor(np.argmax(lg.detach().numpy()[:, :nb], axis=1))
        res = (lg[:, nb:] * (pi / nb)).gather(1, win[:, None])[:, 0]
        return torch.remainder(win.to(tdt) * (2.0 * pi / nb) + res + pi, 2.0 * pi) - pi

    def term(lg, target, k):
        """[tot, ce, rl] of one variant: classes k [B] or [B, B] (given: the float32 rule's), residual continuous in the target"""
        k = torch.as_tensor(k.astype(np.int64)).reshape(target.shape)
        a = torch.remainder(target, twopi)
        sh = a if mutation == "half_bin_shift_dropped" else torch.remainder(a + apc / 2, twopi)
        res = sh - (k.to(tdt) * apc + apc / 2)   # (no value case holds an out-of-range label: the wrap rule shows in the classes of the sweep only)
        k0 = k[:, 0]
        ce = torch.nn.functional.cross_entropy(lg[:, :nb], k0)
        pick = lg[:, nb:].gather(1, k0[:, None])[:, 0]
        err = pick[None, :] - (res / pinb).expand(B, B)
        if mutation == "last_row_slice_dropped" and B >= 64 and B % 64:
            err = err[:64 * (B // 64)]
        h = torch.where(err.abs() <= 1, 0.5 * err * err, err.abs() - 0.5).sum()
        rl = h / (B if mutation == "residual_mean_over_B" else B * B)
        return torch.stack([ce + 20.0 * rl, ce, rl])

    def choose(lg, target, kk):
        x = term(lg, target, kk[0])
        if not ai:
            return x
        y = term(lg, target + pi, kk[1])
        larger = bool(x[0] > y[0])
        if mutation == "cond_picks_smaller":
            larger = not larger
        return x if larger else y
    p1, p2 = decode(ep["pred_pc1angle_logits"]), decode(ep["pred_pc2angle_logits"])
    if mutation == "towers_lose_s3":
        p1, p2 = p1.detach(), p2.detach()
    dth = p2 - p1
    if mutation == "pair_label_column0":
        dth = dth[0].expand(B)
    s1a, s1b = hub(ep["pred_s1_pc1centers"] - c1, 1.0), hub(ep["pred_s1_pc2centers"] - c2, 1.0)
    s2a, s2b = hub(ep["pred_s2_pc1centers"] - c1, 1.0), hub(ep["pred_s2_pc2centers"] - c2, 1.0)
    s3t = hub(ep["pred_translations"] - tr, 1.0 if mutation == "stage3_huber_delta1" else 2.0)
    A1, A2 = choose(ep["pred_pc1angle_logits"], a1, cls[0]), choose(ep["pred_pc2angle_logits"], a2, cls[1])
    A3 = choose(ep["pred_remaining_angle_logits"], (a2 - a1) - dth[None, :], cls[2])
    lt = esf * ((s1a + s1b) / 2 + (s2a + s2b) / 2) + s3t
    la = esf * ((A1[0] + A2[0]) / 2) + A3[0]
    loss = (lt + af * la) / B
    out = torch.stack([loss, lt, la, s1a, s1b, s2a, s2b, s3t, *A1, *A2, *A3]).detach().numpy()
    res = dict(out=out, cls=cls)
    res.update(_grads_of(loss, leaves, case))
    return res
