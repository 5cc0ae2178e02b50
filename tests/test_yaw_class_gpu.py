"""GPU: the yaw class the network itself takes in the middle of its forward pass (csrc/kernels_infer.h stage2_finish_cloud: arg-max over the class logits,
first maximum wins, the residual of THAT class, the wrap into [-pi, pi)), on planted class logits (tests/yaw_cases.py): lone maxima at the first and last
class, exact ties within a lane and across lanes, nb > 64 (a lane holds two classes), nb = 17 (the head's last column tile partial), angles at and beyond
the wrap.  Every forward test elsewhere draws random nets, which decide three of twelve classes and never tie.

Each case first shows that the planted logits reached the kernel bit for bit (the engine returns the floats it maximised over), then compares all eight
outputs of every pair with the UNPINNED fp64 oracle (np.argmax takes the first maximum too) at compare_forward's bars, no pair left out.  tests/
test_yaw_class_cpu.py shows that taking the other tied class would move a stage-3 output by more than 100 x the bar.

No NaN or -inf class logits here: the clamp `if (cls >= nb) cls = 0` behind the arg-max is what keeps such input from indexing out of bounds, and a test of
it would fault the GPU if the clamp were wrong.  By reading: every lane starts at cls = 0x7fffffff and keeps it only if no logit compared greater than
-inf; the cross-lane step takes the smaller index on equal values, so the result is either a class < nb or 0x7fffffff, which the clamp sends to 0."""
import numpy as np
import pytest

import alignnet3d
from tests import yaw_cases as YC
from tests.helpers import compare_forward_all, CLASS_KEYS

pytestmark = pytest.mark.gpu
UKEYS = ("s1_0", "s2_0", "s1_1", "s2_1", "rem")
DG_TRAIN = dict(s1=(32, 64, 96), s2=(32, 64, 128), emb=(64, 128, 160))   # the DGCNN training widths of tests/test_train_gpu.py


def _planted(case):
    nb, cl, res, want, other = YC.CASES[case]
    return np.tile(np.concatenate([cl, res]), (YC.B, 1)), want


def _forward_case(case, backbone, split, tol):
    cfg, spec, P, d = YC.setup(case, backbone=backbone)
    logits, want = _planted(case)
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P)
    if split:
        eng.set_option("infer_matmul_bf16x3", 1)
        assert eng.get_option("infer_matmul_bf16x3") == 1
    ep = eng.forward(d["pcs1"], d["pcs2"])
    kernel = eng.last_backbone_kernel()
    graph = eng.debug_knn_graph(YC.B) if backbone == "dgcnn" else None
    eng.close()
    for k in CLASS_KEYS:
        assert ep[k].dtype == np.float32 and np.array_equal(ep[k].view(np.uint32), logits.view(np.uint32)), "the planted logits did not reach the kernel: " + k
    ref, _, aux = YC.oracle(spec, P, d)
    assert (aux["t1"]["cls"] == want).all() and (aux["t2"]["cls"] == want).all()
    worst, pinned, left_out = compare_forward_all(ep, ref, aux, P, spec, d["pcs1"], d["pcs2"], atol=tol, rtol=tol, knn_graph=graph)
    print("%s %s%s (%s): pinned pairs %d, left out %s, worst abs err %s" % (case, backbone, " split-bf16" if split else "", kernel, pinned, left_out,
                                                                          {k: float("%.2g" % v) for k, v in worst.items()}))
    assert pinned == 0                        # the engine's class is np.argmax of the same floats: the oracle's own
    assert backbone == "dgcnn" or left_out == []


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("case", sorted(YC.CASES))
def test_pointnet_forward_on_planted_class_logits(gpu_required, case, split):
    _forward_case(case, "pointnet", split, 1e-4)


@pytest.mark.parametrize("case", ["nb12_tie_4_9", "nb72_tie_3_64"])
def test_dgcnn_forward_on_planted_class_logits(gpu_required, case):
    """DGCNN, exact fp32, at the 2e-4 bars its forward tests hold (compare_forward_all's kNN allowance: at most one pair's stage 3, and only with the
    near-tie of fp32 distances shown on that pair)."""
    _forward_case(case, "dgcnn", 0, 2e-4)


@pytest.mark.parametrize("backbone", ["pointnet", "dgcnn"])
@pytest.mark.parametrize("case", ["nb12_tie_4_9", "nb72_tie_3_64", "nb12_lone_11", "nb72_lone_70"])
def test_training_forward_decides_the_planted_class(gpu_required, case, backbone):
    """The training forward's decision write-out (Engine.debug_train_decisions "yaw").  With these widths the pointnet step folds the decode into
    stage2_finish_moments_kernel (csrc/kernels_train_dgcnn.h, one wave of a 256-thread workgroup per cloud) and the dgcnn step launches
    stage2_finish_kernel (four clouds per workgroup): both call sites of stage2_finish_cloud."""
    w = DG_TRAIN if backbone == "dgcnn" else {}
    cfg, spec, P, d = YC.setup(case, backbone=backbone, **w)
    logits, want = _planted(case)
    rng = np.random.default_rng(3)
    us = [rng.uniform(size=(YC.B, spec.s2_fc[-1])).astype(np.float32) for _ in UKEYS]
    eng = alignnet3d.Engine(cfg)
    eng.set_variables(P)
    res = eng.train_forward_backward(d["pcs1"], d["pcs2"], d, us)
    yaw = eng.debug_train_decisions(YC.B)["yaw"]
    eng.close()
    for k in CLASS_KEYS:
        assert np.array_equal(np.asarray(res[k], np.float32).view(np.uint32), logits.view(np.uint32)), "the planted logits did not reach the kernel: " + k
    assert np.isfinite(res["loss"])
    np.testing.assert_array_equal(yaw, np.full((2, YC.B), want, np.int32))
