"""Shared helpers for the parity tests (the oracle is the checker, never the product)."""
import numpy as np

from oracle import alignnet_ref as R


def small_cfg(N=128, nb=12, s1=(32, 64, 96), s2=(32, 64, 128), emb=(32, 64, 160), fc=(64, 32), backbone="pointnet"):
    return {
        "data": {"num_channels": 3, "ntrain": 1000},
        "model": {
            "backbone": backbone, "num_points": N,
            "options": {
                "angle_factor": 1.0, "early_stage_factor": 0.5,
                "s1transformer": [list(s1), [list(fc), 0.7]],
                "s2transformer": [list(s2), [list(fc), 0.7]],
                "embedding": list(emb),
                "remaining_transform_prediction": [list(fc), 0.7],
            },
            "angles": {"num_bins": nb, "accept_inverted_angle": True},
        },
        "training": {
            "batch_size": 8, "learning_rate": 0.005, "optimizer": {"optimizer": "adam"},
            "lr_extension": {"mode": "decay", "per": "epoch", "step": 30, "rate": 0.5},
            "bn_extension": {"mode": "decay", "per": "epoch", "step": 30, "rate": 0.5, "init": 0.5, "clip": 0.99},
        },
        "gpu_index": 0,
    }


def oracle_params(cfg, seed=0, bn_seed=1):
    """fp32-representable parameters (what the engine holds), as float64 arrays for the oracle."""
    spec = R.NetSpec.from_cfg(cfg)
    P = R.init_params(spec, seed, np.float32)
    R.randomize_bn(P, bn_seed)
    return spec, {k: v.astype(np.float32) for k, v in P.items()}


def logit_margin(logits, nb):
    s = np.sort(logits[:, :nb], axis=1)
    return s[:, -1] - s[:, -2]


def compare_forward(ep_hip, ep_ref, nb, atol=1e-4, rtol=1e-4, margin_eps=1e-3):
    """Bar (BASELINE.json north_star): outputs within 1e-4 in fp32.  The yaw argmax in the
    middle of the network (models/tp8.py:296) is discontinuous: pairs whose top-2 class-logit
    margin is below margin_eps in either tower are excluded from the stage-3 outputs and counted."""
    m1 = logit_margin(ep_ref["pred_pc1angle_logits"], nb)
    m2 = logit_margin(ep_ref["pred_pc2angle_logits"], nb)
    stable = (m1 > margin_eps) & (m2 > margin_eps)
    worst = {}
    for k in ep_ref:
        a, b = ep_hip[k].astype(np.float64), ep_ref[k].astype(np.float64)
        if k in ("pred_translations", "pred_remaining_angle_logits"):
            a, b = a[stable], b[stable]
        err = np.abs(a - b)
        worst[k] = float(err.max()) if err.size else 0.0
        assert np.all(err <= atol + rtol * np.abs(b)), (k, worst[k])
    return worst, int((~stable).sum())


def varied_pairs(B, N, seed=1234, dtype=np.float32, lo=0.4, hi=1.6):
    """synth_pairs with objects of different size and proportions: every pair's box is stretched by its own U(lo, hi) factor per axis in
    the object frame (both clouds of a pair show the same object; labels unchanged).  Why the tests want it: alignnet3d/synth.py draws ONE
    box shape for every pair, so after stage 3's canonicalisation (models/tp8.py:122-127) all clouds of a batch look alike, the pooled
    features differ between samples only by sampling noise, and the heads' batch normalisation (utils/tf_util.py:455-492) divides by that
    small spread: the fp64 oracle's own gradient then moves by 1e-3 .. 1e-2 when its inputs move by one fp32 rounding
    (tools/pinned_report.py prints it).  Real batches hold different objects; with varied boxes the same perturbation moves the
    gradient by ~1e-5 .. 1e-4, and a sharp bar means something."""
    rng = np.random.default_rng(seed + 77)
    d = {k: v.astype(np.float64) for k, v in R.synth_pairs(B, N, seed=seed, dtype=np.float64).items()}
    sc = rng.uniform(lo, hi, (B, 1, 3))
    for k, c, a in (("pcs1", "pc1_centers", "pc1_angles"), ("pcs2", "pc2_centers", "pc2_angles")):
        p = d[k] - d[c][:, None, :]
        cs, sn = np.cos(d[a][:, 0])[:, None], np.sin(d[a][:, 0])[:, None]
        q = np.stack([p[..., 0] * cs + p[..., 1] * sn, -p[..., 0] * sn + p[..., 1] * cs, p[..., 2]], -1) * sc   # object frame, stretched
        d[k] = np.stack([q[..., 0] * cs - q[..., 1] * sn, q[..., 0] * sn + q[..., 1] * cs, q[..., 2]], -1) + d[c][:, None, :]
    return {k: v.astype(dtype) for k, v in d.items()}


CLASS_KEYS = ("pred_pc1angle_logits", "pred_pc2angle_logits")
STAGE3_KEYS = ("pred_translations", "pred_remaining_angle_logits")


def engine_yaw_classes(ep_hip, nb):
    """The class stage 3 turned by, per tower: stage2_finish_cloud writes out the floats it maximises over and its first maximum wins, which is np.argmax."""
    return [np.argmax(np.asarray(ep_hip[k])[:, :nb], axis=1) for k in CLASS_KEYS]


def knn_near_tie_pairs(graph, pcs1, pcs2, k=20):
    """For compare_forward_all's DGCNN allowance: the pairs in which the engine's fp32 kNN graph (Engine.debug_knn_graph, [2, B, N, k]) lists, for some query,
    another neighbour SET than the fp64 graph (R.knn_indices on the mean-centred cloud) AND every such difference sits at a near-tie: the points listed by one
    side only are all within the fp32 rounding of the distance expression |x|^2 - 2 x.y + |y|^2 of the k-th nearest distance (64 eps32 (|x|^2 + max |y|^2), the
    bound tests/test_forward_gpu.py::test_knn_graph_against_oracle holds the graph to).  Points that are bit-copies of each other are one point here: a
    copy exchanged for a copy changes no edge feature and shows no cause.  Returns a bool [B]."""
    B = len(pcs1)
    out = np.zeros(B, bool)
    for b in range(B):
        differs, near = False, True
        for t, pcs in enumerate((pcs1, pcs2)):
            x = np.asarray(pcs[b], np.float64)
            x = x - x.mean(axis=0, keepdims=True)
            first = {}
            rep = np.array([first.setdefault(tuple(p), i) for i, p in enumerate(np.asarray(pcs[b]).tolist())])   # index of a point's first copy
            want = R.knn_indices(x[None], k)[0]
            sq = (x * x).sum(-1)
            dist = sq[:, None] - 2.0 * x @ x.T + sq[None, :]
            kth = np.sort(dist, axis=1)[:, k - 1]
            eps = 64 * np.finfo(np.float32).eps * (sq + sq.max())
            for q in np.nonzero((np.sort(rep[graph[t, b]], axis=1) != np.sort(rep[want], axis=1)).any(axis=1))[0]:
                ge, go = sorted(rep[graph[t, b, q]]), sorted(rep[want[q]])
                only = [i for i in set(ge) | set(go) if ge.count(i) != go.count(i)]
                differs = True
                near = near and all(abs(dist[q, i] - kth[q]) <= eps[q] for i in only)
        out[b] = differs and near
    return out


def compare_forward_all(ep_hip, ep_ref, aux, P, spec, pcs1, pcs2, atol=1e-4, rtol=1e-4, knn_graph=None):
    """compare_forward without its mask: EVERY pair, all eight outputs.  Given the yaw class the forward is continuous (relu and max are), so the oracle is
    given the class the engine took (engine_yaw_classes) wherever that is not its own, after checking that the class is legitimate:

        yaw_gap = (oracle's top class logit) - (oracle's logit at the engine's class)  <=  tol(c_engine) + tol(c_oracle),   tol(c) = atol + rtol |oracle logit c|.

    The bound follows from the logits comparison below: the engine's winner beats the engine's logit at the oracle's class, and each engine logit lies within
    tol of the oracle's, so the winner cannot trail the oracle's maximum by more than the two tolerances.  It is a consistency check, it drops nothing.
    Pairs whose classes agree are compared against ep_ref as it is, however small the margin; the others against a pinned re-run of the oracle on those pairs
    alone (eval-mode pairs are independent).  ep_ref, aux: R.get_model's unpinned result on (pcs1, pcs2); P: the parameters (any float dtype).
    knn_graph: DGCNN only, the engine's debug_knn_graph of this batch.  Then at most ONE pair may be left out of the stage-3 outputs, and only if
    knn_near_tie_pairs shows the cause on that pair; without it (every pointnet caller) no pair is left out, ever.
    Returns (worst abs error per tensor, number of pinned pairs, list of pairs left out)."""
    nb = spec.num_bins
    assert knn_graph is None or spec.backbone == "dgcnn"
    B = len(pcs1)
    ce = engine_yaw_classes(ep_hip, nb)
    co = [np.asarray(aux["t1"]["cls"]), np.asarray(aux["t2"]["cls"])]
    pin = np.nonzero((ce[0] != co[0]) | (ce[1] != co[1]))[0]
    ref = {k: np.asarray(v, np.float64) for k, v in ep_ref.items()}
    if pin.size:
        P64 = {k: np.asarray(v, np.float64) for k, v in P.items()}
        rp, _, ap = R.get_model(P64, spec, np.asarray(pcs1, np.float64)[pin], np.asarray(pcs2, np.float64)[pin], yaw_cls=(ce[0][pin], ce[1][pin]))
        for t, key in enumerate(CLASS_KEYS):
            lg = ref[key][pin, :nb]
            np.testing.assert_allclose(rp[key], ref[key][pin], rtol=0, atol=1e-9)   # the pin moves nothing in front of stage 3 (a BLAS product may round another way on fewer rows)
            tol = lambda c: atol + rtol * np.abs(lg[np.arange(pin.size), c])
            gap, bound = ap["t%d" % (t + 1)]["yaw_gap"], tol(ce[t][pin]) + tol(co[t][pin])
            assert np.all(gap <= bound), ("yaw_gap: the engine's class is no near-maximum of the oracle's logits", key, pin[gap > bound].tolist(),
                                          gap[gap > bound].tolist(), bound[gap > bound].tolist())
        ref = {k: v.copy() for k, v in ref.items()}
        for k in STAGE3_KEYS:
            ref[k][pin] = rp[k]
    worst, failing = {}, np.zeros(B, bool)
    err = {k: np.abs(np.asarray(ep_hip[k], np.float64) - ref[k]) for k in ref}
    for k in ref:
        if k in STAGE3_KEYS:
            failing |= (err[k] > atol + rtol * np.abs(ref[k])).reshape(B, -1).any(axis=1)
    left_out = []
    if failing.any() and knn_graph is not None:
        shown = knn_near_tie_pairs(knn_graph, pcs1, pcs2, spec.knn_k)
        left_out = [int(b) for b in np.nonzero(failing & shown)[0]][:1]
    keep = np.ones(B, bool)
    keep[left_out] = False
    for k in ref:
        e, r = (err[k][keep], ref[k][keep]) if k in STAGE3_KEYS else (err[k], ref[k])
        worst[k] = float(e.max()) if e.size else 0.0
        assert np.all(e <= atol + rtol * np.abs(r)), (k, worst[k], "pairs", np.nonzero((e > atol + rtol * np.abs(r)).reshape(len(e), -1).any(axis=1))[0].tolist())
    return worst, int(pin.size), left_out
