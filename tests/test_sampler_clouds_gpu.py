"""GPU: the network on clouds as the batch sampler draws them (tests/sampler_cases.py): bit-identical copies of points, tiny clouds, empty clouds.
Every other network test draws N distinct points, so until here no test ran knn_kernel's 4b / 4c select paths (tests/test_sampler_clouds_cpu.py proves
which queries of these inputs do), and no live max-pool channel ever held an exact tie.

  * the kNN graph (eval forward and training forward) against the fp64 oracle: tests/knn_select_ref.py check_rows;
  * eval forward against the fp64 oracle at the bars of tests/test_forward_gpu.py, every pair alone bit-identical to the pair in the batch;
  * training: the max-pools' "first copy wins" (exact), the decision-pinned gradient check of tests/test_train_gpu.py on sampler batches, one unpinned
    gradient check per backbone (torch's amax splits a tie evenly, the engine routes it to the first copy: the weight gradients agree, a backward that
    found winners by value would double-count), and a batch whose second tower is empty."""
import numpy as np
import pytest

import alignnet3d
from oracle import alignnet_ref as R
from tests import knn_select_ref as KS
from tests import sampler_cases as SC
from tests.helpers import small_cfg, oracle_params, compare_forward, compare_forward_all
from tests.test_train_gpu import (DGCNN_GENERAL, PINNED_CASES, STD, _grad_check, _oracle, pinned_check)

pytestmark = pytest.mark.gpu
K = KS.K
UKEYS = ("s1_0", "s2_0", "s1_1", "s2_1", "rem")
SCOPES = ("transformer1/embedding", "transformer2/embedding", "embedding")


def _rows(B):
    """B dataset rows: the mixed batch first (an empty tower on either side, both empty, tiny, about 300, larger than N), then the other pairs."""
    return list(range(len(SC.ROWS)))[:B]


def _uniforms(B, seed=13):
    rng = np.random.default_rng(seed)
    return {k: rng.uniform(size=(B, 32)).astype(np.float32) for k in UKEYS}


# ---------------------------------------------------------------- kNN graph ----------------------------------------------------------------
@pytest.mark.parametrize("N", SC.KNN_SIZES)
def test_knn_graph_on_sampler_clouds(gpu_required, N):
    """knn_kernel<16> / <32> / <64> on clouds that put hundreds of queries on each of 4a, 4b and 4c (proved on the CPU), through alignnet_debug_knn_graph after
    an eval forward and ALIGNNET_DECISION_KNN_GRAPH after a training forward.  Every decided row equals R.knn_indices (fp64, mean-centred cloud) as a set; rows
    are nearest-first where the restatement says 4a and (nearer, then ties at rank k) x index order elsewhere; within the tie group at rank k the listed copies
    are the lowest indices; the all-zero cloud gives rows 0..19; a pair alone gives the rows it gives in a batch large enough to change the queries per
    workgroup.  Undecided queries (another unique point within the fp32 rounding of the rank-k distance): at most 1e-3 of a cloud of at most 60 unique points."""
    rows = SC.knn_rows(N)
    B = len(rows)
    d = SC.batch(rows, N)
    cfg = small_cfg(N=N, backbone="dgcnn")
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    reps = 1
    while KS.queries_per_workgroup(B * reps, N) == KS.queries_per_workgroup(1, N):
        reps += 1
    eng.forward(np.tile(d["pcs1"], (reps, 1, 1)), np.tile(d["pcs2"], (reps, 1, 1)))
    g = eng.debug_knn_graph(B * reps)
    assert g.shape == (2, B * reps, N, K)
    for r in range(1, reps):
        np.testing.assert_array_equal(g[:, r * B:(r + 1) * B], g[:, :B])
    g = g[:, :B]
    for b in range(B):                                                     # every pair alone: other grid, other queries per workgroup, same rows
        eng.forward(d["pcs1"][b:b + 1], d["pcs2"][b:b + 1])
        np.testing.assert_array_equal(eng.debug_knn_graph(1)[:, 0], g[:, b], err_msg="pair %d alone" % b)
    eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [_uniforms(B)[k] for k in UKEYS])
    gt = eng.debug_train_decisions(B)["knn"]
    eng.close()
    count, undecided = {p: 0 for p in "abc"}, {}
    for t, key in enumerate(("pcs1", "pcs2")):
        uniq = SC.unique_points(rows, t)
        for b in range(B):
            pc = d[key][b]
            _, path, _ = KS.select(pc, rows=False)
            for p in "abc":
                count[p] += int((path == p).sum())
            orc = KS.oracle(pc)
            und = KS.check_rows(g[t, b], pc, path=path, orc=orc)
            if not np.array_equal(gt[t, b], g[t, b]):                      # (the same kernel on the same cloud: the training graph is the eval graph, or is judged alike)
                KS.check_rows(gt[t, b], pc, path=path, orc=orc)
            undecided[(rows[b], t, uniq[b])] = und
            if uniq[b] <= 60:
                assert und <= 1e-3 * N, (rows[b], t, uniq[b], und)
            if uniq[b] == 0:
                np.testing.assert_array_equal(g[t, b], np.tile(np.arange(K), (N, 1)))
                np.testing.assert_array_equal(gt[t, b], np.tile(np.arange(K), (N, 1)))
    print("kNN on sampler clouds, N=%d, batch %d x %d: queries per path (restated) %s; undecided queries per (row, tower, unique points): %s" % (
        N, B, reps, count, {k: v for k, v in undecided.items() if v}))
    assert min(count.values()) >= 100


# ---------------------------------------------------------------- eval forward ----------------------------------------------------------------
def _forward_and_alone(cfg, P32, d, options):
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    for k, v in options:
        eng.set_option(k, v)
        assert eng.get_option(k) == v
    ep = eng.forward(d["pcs1"], d["pcs2"])
    kernel = eng.last_backbone_kernel()
    graph = eng.debug_knn_graph(len(d["pcs1"])) if cfg["model"]["backbone"] == "dgcnn" else None
    for b in range(len(d["pcs1"])):
        alone = eng.forward(d["pcs1"][b:b + 1], d["pcs2"][b:b + 1])
        for k in ep:
            np.testing.assert_array_equal(alone[k][0], ep[k][b], err_msg="pair %d alone: %s" % (b, k))
    eng.close()
    return ep, kernel, graph


def _all_pairs(what, ep, ref, aux, P32, spec, d, atol=1e-4, rtol=1e-4, graph=None):
    """Every pair against the oracle, pinned to the engine's yaw class where the two differ (tests/helpers.py compare_forward_all): pointnet leaves no pair
    out; DGCNN at most one pair's stage 3, with the near-tie of the fp32 kNN distances shown on it."""
    worst, pinned, left_out = compare_forward_all(ep, ref, aux, P32, spec, d["pcs1"], d["pcs2"], atol=atol, rtol=rtol, knn_graph=graph)
    print("%s: ALL %d pairs, %d pinned to the engine's yaw class, left out %s, worst abs err %.2e" % (what, len(d["pcs1"]), pinned, left_out, max(worst.values())))
    assert graph is not None or left_out == []


@pytest.fixture(scope="module")
def forward_ref():
    """fp64 oracle outputs per (backbone, N), computed once."""
    cache = {}

    def get(backbone, N):
        if (backbone, N) not in cache:
            if backbone == "pointnet":
                cfg = alignnet3d.default_model_config()          # the shipped widths: the instantiations serving runs
                cfg["model"]["num_points"] = N
            else:
                cfg = small_cfg(N=N, backbone="dgcnn")
            spec, P32 = oracle_params(cfg)
            d = SC.batch(SC.MIXED, N)
            ref, _, aux = R.get_model({k: v.astype(np.float64) for k, v in P32.items()}, spec, d["pcs1"].astype(np.float64), d["pcs2"].astype(np.float64))
            cache[(backbone, N)] = (cfg, spec, P32, d, ref, aux)
        return cache[(backbone, N)]
    return get


@pytest.mark.parametrize("N", [128, 200])
def test_forward_pointnet_on_sampler_batch(gpu_required, forward_ref, N):
    """The mixed batch (B = 8) against the fp64 oracle at compare_forward's bars (1e-4): exact fp32 on both tile shapes, split-bf16 tile-wise and persistent
    (bit-identical to each other); every pair alone bit-identical to the pair in the batch."""
    cfg, spec, P32, d, ref, aux = forward_ref("pointnet", N)
    B = len(SC.MIXED)
    for tile, kernel in ((128, "pointnet_fused<64,128,k16>"), (64, "pointnet_fused<64,128,k16,tp64>")):
        ep, ran, _ = _forward_and_alone(cfg, P32, d, (("infer_tile_points", tile),))
        assert ran == kernel, ran
        worst, unstable = compare_forward(ep, ref, spec.num_bins)
        print("pointnet fp32 tile %d N=%d: worst abs err %.2e, unstable pairs %d" % (tile, N, max(worst.values()), unstable))
        assert unstable <= max(1, B // 4)
        _all_pairs("pointnet fp32 tile %d N=%d" % (tile, N), ep, ref, aux, P32, spec, d)
    out = {}
    for tilewise, kernel in ((1, "pointnet_split<64,128>"), (0, "pointnet_split_persist")):
        out[tilewise], ran, _ = _forward_and_alone(cfg, P32, d, (("infer_matmul_bf16x3", 1), ("ab_split_tilewise", tilewise)))
        assert ran == kernel, ran
        worst, unstable = compare_forward(out[tilewise], ref, spec.num_bins)
        print("pointnet split-bf16 %s N=%d: worst abs err %.2e, unstable pairs %d" % (kernel, N, max(worst.values()), unstable))
        assert unstable <= max(1, B // 4)
        _all_pairs("pointnet split-bf16 %s N=%d" % (kernel, N), out[tilewise], ref, aux, P32, spec, d)
    for k in out[0]:
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("N", [128, 200])
def test_forward_dgcnn_on_sampler_batch(gpu_required, forward_ref, N, split):
    """DGCNN, exact fp32 and split-bf16, at the bars the DGCNN forward tests hold (compare_forward at 2e-4: the oracle rebuilds the graph per stage in fp64, the
    engine once in fp32).  Among copies the neighbour SET is not unique in the oracle (its sort sees 1e-16 noise between copies), but the max over the k
    neighbours does not see which copies were taken."""
    cfg, spec, P32, d, ref, aux = forward_ref("dgcnn", N)
    ep, ran, graph = _forward_and_alone(cfg, P32, d, (("infer_matmul_bf16x3", split),))
    worst, unstable = compare_forward(ep, ref, spec.num_bins, atol=2e-4, rtol=2e-4)
    print("dgcnn %s N=%d (%s): worst abs err %.2e, unstable pairs %d" % ("split-bf16" if split else "fp32", N, ran, max(worst.values()), unstable))
    assert unstable <= max(1, len(SC.MIXED) // 4)
    _all_pairs("dgcnn %s N=%d" % ("split-bf16" if split else "fp32", N), ep, ref, aux, P32, spec, d, atol=2e-4, rtol=2e-4, graph=graph)


# ---------------------------------------------------------------- training ----------------------------------------------------------------
HYBRID = dict(s1=(48, 96, 160), s2=(32, 32, 32, 64, 128), emb=(40, 72, 104))   # a hybrid stage, a five-layer stage with a fused tail, a stage no fused kernel fits
FIRST_COPY = {
    # name: (backbone, widths, N, B, options)
    "fused": ("pointnet", dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(32, 64, 160)), 128, 8, ()),
    "fused_std_parts1": ("pointnet", STD, 200, 12, (("pn_cloud_parts", 1),)),
    "fused_std_parts2": ("pointnet", STD, 200, 12, (("pn_cloud_parts", 2),)),
    "fused_std_parts4": ("pointnet", STD, 200, 12, (("pn_cloud_parts", 4),)),
    "fused_std_tile64": ("pointnet", STD, 200, 12, (("train_phase3_tile64", 1), ("pn_cloud_parts", 1))),
    "hybrid": ("pointnet", HYBRID, 128, 8, (("train_fused_tail", 1),)),
    "layerwise": ("pointnet", HYBRID, 200, 5, (("train_fused_tail", 0),)),
    "dgcnn": ("dgcnn", dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(64, 128, 160)), 128, 8, ()),
    "dgcnn_std_parts1": ("dgcnn", STD, 200, 6, (("dg_cloud_parts", 1), ("pn_cloud_parts", 1))),
    "dgcnn_std_parts2": ("dgcnn", STD, 200, 6, (("dg_cloud_parts", 2), ("pn_cloud_parts", 2))),
    "dgcnn_std_parts4": ("dgcnn", STD, 200, 6, (("dg_cloud_parts", 4), ("pn_cloud_parts", 4))),
    "dgcnn_layerwise": ("dgcnn", DGCNN_GENERAL["mixed"], 128, 5, ()),
}


@pytest.mark.parametrize("case", sorted(FIRST_COPY))
def test_pool_winners_are_first_copies(gpu_required, case):
    """"First maximum wins" (kernels_train_fwd.h, kernels_train_generic.h, kernels_train_dgcnn.h), exact: with copies in the cloud every channel's maximum is
    an exact tie between all copies of the winner -- across the 64 / 128-point tiles and across the workgroups a cloud is dealt to -- and the winner must be
    the copy of lowest index; for the max over the k neighbour slots, the lowest slot of the step's graph row that holds a copy.  (A rigid motion of the whole
    cloud keeps bit-copies bit-copies, so the classes of the raw batch are those of every stage's frame.)  The batch makes the rule bite: in most LIVE channels
    (relu on at the winner) the winner has more than one copy.
    Not under train_matmul_bf16: there the maximum is taken over keys -- the value with its low four mantissa bits replaced by the accumulator register number
    (kernels_train_fwd.h, layer 3) -- so among copies the register number decides, by design (measured: 39 of 96 channels of an all-zero cloud go to point 27);
    that mode's winners are held to the oracle's values by the pinned test below."""
    backbone, w, N, B, options = FIRST_COPY[case]
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), backbone=backbone, **w)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=13)
    d = SC.batch(_rows(B), N)
    pcs = (d["pcs1"], d["pcs2"])
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    for k, v in options:
        eng.set_option(k, v)
        assert eng.get_option(k) == v
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [_uniforms(B)[k] for k in UKEYS])
    dec = eng.debug_train_decisions(B, relu=True)
    eng.close()
    assert np.isfinite(res["loss"])
    o = cfg["model"]["options"]
    depth = [len(o["s1transformer"][0]), len(o["s2transformer"][0]), len(o["embedding"])]
    tied = {}
    for s in range(3):
        copies = SC.check_pool_first_copy(dec["pool"][s], pcs)
        live = np.stack([dec["relu"]["%d:%s/conv%d" % (t, SCOPES[s], depth[s])] for t in range(2)])
        tied["pool%d" % s] = float((copies > 1)[live].mean())
        if backbone == "dgcnn":
            copies = SC.check_slot_first_copy(dec["slot"][s], dec["knn"], pcs)
            live = np.stack([dec["relu"]["%d:%s/conv%d" % (t, SCOPES[s], depth[s] - 1)] for t in range(2)]).reshape(copies.shape)
            tied["slot%d" % s] = float((copies > 1)[live].mean())
    print(case, "first-copy rule holds; live channels whose winner has more than one copy:", {k: round(v, 3) for k, v in tied.items()})
    assert all(v > 0.5 for v in tied.values()), tied


SAMPLER_PINNED = {
    # case of tests/test_train_gpu.py PINNED_CASES: (N, B) on the sampler's batch
    "pointnet": (200, 16),
    "pointnet_deep_layerwise": (128, 5),
    "pointnet_std_bf16": (200, 16),
    "dgcnn": (128, 8),
    "dgcnn_std_bf16": (128, 16),
}


@pytest.mark.parametrize("case", sorted(SAMPLER_PINNED))
def test_gradients_match_pinned_autograd_on_sampler_batch(gpu_required, case):
    """tests/test_train_gpu.py::test_gradients_match_autograd_with_pinned_decisions, its assertions and bars unchanged, on a batch as the sampler draws it."""
    backbone, w, _, _, bf16, tail = PINNED_CASES[case]
    N, B = SAMPLER_PINNED[case]
    pinned_check(case + " on a sampler batch", (backbone, w, N, B, bf16, tail), SC.batch(_rows(B), N))


@pytest.mark.parametrize("backbone,N,B,tol", [("pointnet", 200, 16, 5e-4), ("dgcnn", 128, 8, 2e-3)])
def test_gradients_match_unpinned_autograd_on_sampler_batch(gpu_required, backbone, N, B, tol):
    """The oracle deciding for itself: torch's amax splits the gradient of an exact tie evenly among the copies, the engine sends it to the first copy.  The
    copies' inputs are identical, so every weight gradient agrees; a backward that routed to every equal maximum would count a channel once per copy.
    Criterion and bars of test_gradients_match_autograd (B = 16: 5e-4) / test_dgcnn_gradients_match_autograd (N = 128, B = 8: 2e-3)."""
    w = dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(32, 64, 160) if backbone == "pointnet" else (64, 128, 160))
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), backbone=backbone, **w)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=5)
    d, du = SC.batch(_rows(B), N), _uniforms(B, 5)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in UKEYS])
    _, loss_ref, grads, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"])
    bad, worst = _grad_check(eng, spec, grads, tol)
    print(backbone, "unpinned oracle on a sampler batch: loss %.7f / %.7f, worst relative gradient error %.2e" % (res["loss"], loss_ref, worst))
    eng.close()
    assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    assert not bad, bad


@pytest.mark.parametrize("backbone", ["pointnet", "dgcnn"])
def test_batch_with_an_empty_tower_trains(gpu_required, backbone):
    """Every cloud of tower 2 empty: B x N points at the origin, so every BatchNorm of that tower sees zero variance and every max an all-way tie.  Predictions,
    loss and every gradient against the pinned oracle (bars of the B = 6 cases of tests/test_train_gpu.py: 2e-4, 1e-4, 1e-2 -- the gradient bar widened, per tensor,
    to twice the fp32 evaluation of the oracle's own error where zero variance makes fp32 itself lose the tensor), then a full optimiser step: finite."""
    N, B = 128, len(SC.TOWER2_EMPTY)
    w = dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(32, 64, 160) if backbone == "pointnet" else (64, 128, 160))
    cfg = small_cfg(N=N, nb=12, fc=(64, 32), backbone=backbone, **w)
    cfg["training"]["batch_size"] = B
    spec, P32 = oracle_params(cfg, seed=5)
    d, du = SC.batch(SC.TOWER2_EMPTY, N), _uniforms(B, 5)
    assert not d["pcs2"].any()
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P32)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, [du[k] for k in UKEYS])
    dec = eng.debug_train_decisions(B, relu=True)
    ep_ref, loss_ref, grads, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], pinned=dec)
    for s in range(3):
        assert not dec["pool"][s][1].any(), "empty clouds: every point ties, point 0 wins"
        if backbone == "dgcnn":
            assert not dec["slot"][s][1].any(), "empty clouds: every neighbour slot ties, slot 0 wins"
    if backbone == "dgcnn":
        np.testing.assert_array_equal(dec["knn"][1], np.broadcast_to(np.arange(K), (B, N, K)))
    for k in ep_ref:
        assert np.isfinite(res[k]).all(), k
        np.testing.assert_allclose(res[k], ep_ref[k], rtol=2e-4, atol=2e-4, err_msg=k)
    assert abs(res["loss"] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (res["loss"], loss_ref)
    for n in R.trainable_names(spec):
        assert np.isfinite(eng.get_gradient(n)).all(), n
    # Gradients.  Three BatchNorms of zero variance in a row multiply a gradient by up to (gamma / sqrt(eps))^3 = 3e4 before sums that are exactly zero in
    # exact arithmetic (the rows of a constant column see dy - mean(dy)) cancel it again: no fp32 evaluation resolves those sums -- the reference graph itself,
    # evaluated by torch in fp32 with the same pinned decisions, is off by 2.6 x its largest entry on stage 1's second conv (measured on the CPU; fp64: 1e-12).
    # Bar per tensor: the B = 6 bar of tests/test_train_gpu.py (1e-2 of the tensor's largest entry + 1e-5 of the gradient's), or twice the fp32 oracle's own
    # error on that tensor where that is larger (the rule of test_dgcnn_general_widths_and_depth_train).  A bias in front of a BatchNorm: exactly 0 in the engine.
    _, _, g32, _ = _oracle(cfg, P32, d, du, eng.state()["bn_decay"], dt=np.float32, pinned=dec)
    gscale = max(float(np.abs(v).max()) for v in grads.values())
    bn_bias = {(f"siamese/{L.name}" if L.siamese else L.name) + "/biases" for L in R.layer_table(spec) if L.bn}
    bad, worst, worst32 = {}, 0.0, 0.0
    for name in R.trainable_names(spec):
        g = eng.get_gradient(name).astype(np.float64)
        ref = grads[name].reshape(g.shape)
        if name in bn_bias:
            assert np.abs(g).max() == 0.0, name
            continue
        err, top = float(np.abs(g - ref).max()), float(np.abs(ref).max())
        own32 = float(np.abs(g32[name].astype(np.float64).reshape(g.shape) - ref).max())
        worst, worst32 = max(worst, err / (top + 1e-6 * gscale)), max(worst32, own32 / (top + 1e-6 * gscale))
        if err > max(1e-2 * top + 1e-5 * gscale, 2.0 * own32):
            bad[name] = (err, top, own32)
    print(backbone, "tower 2 empty: loss %.7f / %.7f, worst relative gradient error %.2e (the fp32 oracle's own: %.2e)" % (res["loss"], loss_ref, worst, worst32))
    assert not bad, bad
    r = eng.train_step(d["pcs1"], d["pcs2"], d)
    assert r["step"] == 1 and np.isfinite(r["loss"])
    for n, _, _ in eng.variables():
        assert np.isfinite(eng.get_variable(n)).all(), n
    eng.close()
