"""CPU: the oracle's optional pinned yaw class (oracle/alignnet_ref.py get_angles / embedding_net / get_model), the planted cases of tests/yaw_cases.py
and tests/helpers.py compare_forward_all, without a GPU."""
import numpy as np
import pytest

from oracle import alignnet_ref as R
from tests import yaw_cases as YC
from tests.helpers import small_cfg, oracle_params, compare_forward_all, logit_margin, CLASS_KEYS, STAGE3_KEYS

FRONT = ("pred_s1_pc1centers", "pred_s1_pc2centers", "pred_s2_pc1centers", "pred_s2_pc2centers") + CLASS_KEYS
BAR = 1e-4   # compare_forward's


@pytest.fixture(scope="module")
def net():
    """small_cfg, N = 100, B = 3 (a shape tests/test_forward_gpu.py runs): parameters, clouds and the unpinned oracle result."""
    cfg = small_cfg(N=100)
    spec, P32 = oracle_params(cfg)
    d = R.synth_pairs(3, 100, seed=1234, dtype=np.float32)
    ep, _, aux = YC.oracle(spec, P32, d)
    return spec, P32, d, ep, aux


def _runner_up(ep, nb):
    return [np.argsort(-ep[k][:, :nb], axis=1, kind="stable")[:, 1] for k in CLASS_KEYS]


def test_pinning_to_own_classes_changes_no_bit(net):
    spec, P32, d, ep, aux = net
    for yaw in ((aux["t1"]["cls"], aux["t2"]["cls"]), (aux["t1"]["cls"].astype(np.int32), None), (None, list(aux["t2"]["cls"]))):
        ep2, _, aux2 = YC.oracle(spec, P32, d, yaw_cls=yaw)
        for k in ep:
            np.testing.assert_array_equal(ep2[k], ep[k], err_msg=k)
        for t in ("t1", "t2"):
            np.testing.assert_array_equal(aux2[t]["cls"], aux[t]["cls"])
            np.testing.assert_array_equal(aux2[t]["ang"], aux[t]["ang"])
            assert not aux2[t]["yaw_gap"].any() and not aux[t]["yaw_gap"].any()


def test_get_angles_takes_the_class_it_is_given():
    nb = 12
    lg = np.random.default_rng(0).normal(size=(5, 2 * nb))
    a0, c0 = R.get_angles(lg, nb)
    a1, c1 = R.get_angles(lg, nb, cls=c0)
    np.testing.assert_array_equal(a0, a1)
    np.testing.assert_array_equal(c0, c1)
    c = (c0 + 5) % nb
    a2, c2 = R.get_angles(lg, nb, cls=c)
    np.testing.assert_array_equal(c2, c)
    pi = float(np.float32(np.pi))
    want = c * (2 * pi / nb) + lg[np.arange(5), nb + c] * (pi / nb)
    turns = (a2 - want) / (2 * pi)                      # the graph's period is 2 x float32(pi)
    np.testing.assert_allclose(turns, np.round(turns), rtol=0, atol=1e-12)
    assert ((a2 >= -pi) & (a2 < pi)).all()


def test_pinning_one_pair_to_its_runner_up_moves_stage_3_only(net):
    spec, P32, d, ep, aux = net
    nb = spec.num_bins
    ru = _runner_up(ep, nb)
    b = 1
    c1 = aux["t1"]["cls"].copy()
    c1[b] = ru[0][b]
    ep2, _, aux2 = YC.oracle(spec, P32, d, yaw_cls=(c1, None))
    for k in FRONT:
        np.testing.assert_array_equal(ep2[k], ep[k], err_msg=k)
    margin = logit_margin(ep["pred_pc1angle_logits"], nb)
    want = np.zeros(3)
    want[b] = margin[b]
    np.testing.assert_array_equal(aux2["t1"]["yaw_gap"], want)
    assert not aux2["t2"]["yaw_gap"].any()
    others = [i for i in range(3) if i != b]
    for k in STAGE3_KEYS:
        np.testing.assert_array_equal(ep2[k][others], ep[k][others], err_msg=k)    # eval-mode pairs are independent
        assert np.abs(ep2[k][b] - ep[k][b]).max() > 100 * BAR, k


@pytest.mark.parametrize("case", sorted(YC.CASES))
def test_planted_logits_reach_the_oracle_exactly(case):
    nb, cl, res, want, other = YC.CASES[case]
    cfg, spec, P, d = YC.setup(case)
    ep, _, aux = YC.oracle(spec, P, d)
    for t, k in enumerate(CLASS_KEYS):
        np.testing.assert_array_equal(ep[k], np.tile(np.concatenate([cl, res]).astype(np.float64), (YC.B, 1)))
        np.testing.assert_array_equal(aux["t%d" % (t + 1)]["cls"], np.full(YC.B, want))
    assert len(set(res.tolist())) == nb, "a residual per class"
    assert all(np.isfinite(v).all() for v in ep.values())


@pytest.mark.parametrize("case", YC.TIES)
def test_planted_ties_have_teeth(case):
    """Had the other tied class been taken, a stage-3 output would move by at least 100 x the bar the GPU test holds, on every pair (measured on the
    least-moved pair: 1.6e-2 .. 7.3e-2, 163 x the bar or more)."""
    cfg, spec, P, d = YC.setup(case)
    tie, _, _ = YC.oracle(spec, P, d)
    cfg, spec, P2, d = YC.setup(case, cls_logits=YC.other_wins(case))
    oth, _, aux = YC.oracle(spec, P2, d)
    assert (aux["t1"]["cls"] == YC.CASES[case][4]).all() and (aux["t2"]["cls"] == YC.CASES[case][4]).all()
    moved = {k: float(np.abs(tie[k] - oth[k]).reshape(YC.B, -1).max(axis=1).min()) for k in STAGE3_KEYS}     # the least-moved pair
    print(case, "least-moved pair, other tied class taken:", moved)
    assert max(moved.values()) >= 100 * BAR, moved
    # the same through the pin: the other class pinned on the tie's own parameters
    pin = np.full(YC.B, YC.CASES[case][4])
    pinned, _, aux = YC.oracle(spec, P, d, yaw_cls=(pin, pin))
    assert not aux["t1"]["yaw_gap"].any() and not aux["t2"]["yaw_gap"].any(), "an exact tie: the other class is a maximum too"
    for k in STAGE3_KEYS:
        np.testing.assert_allclose(pinned[k], oth[k], rtol=0, atol=1e-12, err_msg=k)


def _near_tie_net():
    """The fixture's net with the stage-2 head's bias at pair 0 / tower 1's top class lowered until its margin is 2e-5: a near-tie an fp32 engine decides either way."""
    cfg = small_cfg(N=100)
    spec, P32 = oracle_params(cfg)
    d = R.synth_pairs(3, 100, seed=1234, dtype=np.float32)
    ep, _, aux = YC.oracle(spec, P32, d)
    nb = spec.num_bins
    top = int(aux["t1"]["cls"][0])
    P = {k: v.astype(np.float64) for k, v in P32.items()}
    b = P[YC.last_fc(spec) + "/biases"].copy()
    b[3 + top] -= logit_margin(ep["pred_pc1angle_logits"], nb)[0] - 2e-5
    P[YC.last_fc(spec) + "/biases"] = b
    ep, _, aux = R.get_model(P, spec, d["pcs1"].astype(np.float64), d["pcs2"].astype(np.float64))
    assert abs(logit_margin(ep["pred_pc1angle_logits"], nb)[0] - 2e-5) < 1e-9 and aux["t1"]["cls"][0] == top
    return spec, P, d, ep, aux


def test_compare_forward_all_pins_a_near_tie_and_refuses_a_far_class():
    spec, P, d, ep, aux = _near_tie_net()
    nb = spec.num_bins
    ru = int(_runner_up(ep, nb)[0][0])
    # the oracle's own outputs: nothing to pin, every pair compared
    worst, pinned, left = compare_forward_all(ep, ep, aux, P, spec, d["pcs1"], d["pcs2"])
    assert pinned == 0 and left == [] and max(worst.values()) == 0.0
    # an "engine" that decided pair 0's near-tie the other way, consistently: its logit at the runner-up 3e-5 higher (inside the bar), stage 3 turned by it
    c1 = aux["t1"]["cls"].copy()
    c1[0] = ru
    alt, _, _ = R.get_model(P, spec, d["pcs1"].astype(np.float64), d["pcs2"].astype(np.float64), yaw_cls=(c1, None))
    fake = {k: v.copy() for k, v in alt.items()}
    fake["pred_pc1angle_logits"][0, ru] += 3e-5
    assert np.abs(alt["pred_translations"][0] - ep["pred_translations"][0]).max() > 10 * BAR     # (so that the wrong stage 3 below is far outside the bar)
    worst, pinned, left = compare_forward_all(fake, ep, aux, P, spec, d["pcs1"], d["pcs2"])
    assert pinned == 1 and left == [] and max(worst[k] for k in STAGE3_KEYS) < 1e-9
    # the same logits with the stage 3 of the oracle's own class: the helper pins to the class the logits name, and stage 3 fails
    wrong = {k: v.copy() for k, v in fake.items()}
    for k in STAGE3_KEYS:
        wrong[k] = ep[k].copy()
    with pytest.raises(AssertionError, match="pred_translations|pred_remaining_angle_logits"):
        compare_forward_all(wrong, ep, aux, P, spec, d["pcs1"], d["pcs2"])
    # a class that is no near-maximum: refused by the gap check, whatever stage 3 holds
    far = int(np.argmin(ep["pred_pc1angle_logits"][0, :nb]))
    c1[0] = far
    alt, _, auxf = R.get_model(P, spec, d["pcs1"].astype(np.float64), d["pcs2"].astype(np.float64), yaw_cls=(c1, None))
    assert auxf["t1"]["yaw_gap"][0] > 100 * BAR
    fake = {k: v.copy() for k, v in alt.items()}
    fake["pred_pc1angle_logits"][0, far] = ep["pred_pc1angle_logits"][0, :nb].max() + 1e-5
    with pytest.raises(AssertionError, match="yaw_gap"):
        compare_forward_all(fake, ep, aux, P, spec, d["pcs1"], d["pcs2"])
    # and no pointnet pair may be excused through the kNN allowance
    with pytest.raises(AssertionError):
        compare_forward_all(ep, ep, aux, P, spec, d["pcs1"], d["pcs2"], knn_graph=np.zeros((2, 3, 100, 20), np.int32))


def test_knn_near_tie_pairs_shows_a_near_tie_and_nothing_else():
    """compare_forward_all's DGCNN allowance rests on knn_near_tie_pairs: the fp64 graph itself shows no cause; a row whose 20th neighbour is exchanged for a
    21st that fp32 cannot tell from it does; the same exchange for a far point does not; a copy exchanged for a copy does not."""
    from tests.helpers import knn_near_tie_pairs
    k, N = 20, 48
    rng = np.random.default_rng(11)
    pcs = rng.normal(size=(2, 2, N, 3)).astype(np.float32)            # [tower, pair, point, xyz]
    q = 5
    order = np.argsort(((pcs[0, 0] - pcs[0, 0, q]) ** 2).sum(-1).astype(np.float64), kind="stable")
    a, b = order[k - 1], order[k]
    v = (pcs[0, 0, b] - pcs[0, 0, q]).astype(np.float64)
    ra = np.linalg.norm((pcs[0, 0, a] - pcs[0, 0, q]).astype(np.float64))
    pcs[0, 0, b] = (pcs[0, 0, q] + v * (ra / np.linalg.norm(v))).astype(np.float32)     # b at a's distance from q, to fp32 rounding of the coordinates
    pcs[1, 1, 7] = pcs[1, 1, 3]                                       # pair 1, tower 2: point 7 is a bit-copy of point 3

    def fp64_graph():
        return np.stack([np.stack([R.knn_indices((lambda x: x - x.mean(0))(pcs[t, p].astype(np.float64))[None], k)[0] for p in range(2)]) for t in range(2)])
    g = fp64_graph()
    assert not knn_near_tie_pairs(g, pcs[0], pcs[1], k).any()
    row = g[0, 0, q]
    assert (a in row) != (b in row), "the planted pair straddles rank k"
    inside, outside = (a, b) if a in row else (b, a)
    near = g.copy()
    near[0, 0, q, list(row).index(inside)] = outside
    np.testing.assert_array_equal(knn_near_tie_pairs(near, pcs[0], pcs[1], k), [True, False])
    far = g.copy()
    far[0, 0, q, list(row).index(inside)] = order[-1]
    assert not knn_near_tie_pairs(far, pcs[0], pcs[1], k).any()
    both = near.copy()                                                 # a near-tie AND a far exchange in the same pair: not excused
    both[1, 0, 0, k - 1] = np.argsort(((pcs[1, 0] - pcs[1, 0, 0]) ** 2).sum(-1))[-1]
    assert not knn_near_tie_pairs(both, pcs[0], pcs[1], k).any()
    copies = g.copy()
    rows3 = [r for r in range(N) if (3 in g[1, 1, r]) != (7 in g[1, 1, r])]
    for r in rows3:                                                    # rows that list one of the two copies: list the other one instead
        j = [i for i, x in enumerate(g[1, 1, r]) if x in (3, 7)][0]
        copies[1, 1, r, j] = 10 - g[1, 1, r, j]
    assert not knn_near_tie_pairs(copies, pcs[0], pcs[1], k).any()


def test_dgcnn_allowance_needs_the_cause_shown():
    """A DGCNN pair whose stage 3 is off while its graph is the fp64 graph is not excused: the allowance asks for the near-tie on that very pair."""
    cfg = small_cfg(N=64, backbone="dgcnn")
    spec, P32 = oracle_params(cfg)
    d = R.synth_pairs(2, 64, seed=3, dtype=np.float32)
    ep, _, aux = YC.oracle(spec, P32, d)
    g = np.stack([R.knn_indices((lambda x: x - x.mean(1, keepdims=True))(d[k].astype(np.float64)), spec.knn_k) for k in ("pcs1", "pcs2")])
    worst, pinned, left = compare_forward_all(ep, ep, aux, P32, spec, d["pcs1"], d["pcs2"], atol=2e-4, rtol=2e-4, knn_graph=g)
    assert pinned == 0 and left == []
    off = {k: v.copy() for k, v in ep.items()}
    off["pred_translations"][0] += 1e-2
    with pytest.raises(AssertionError, match="pred_translations"):
        compare_forward_all(off, ep, aux, P32, spec, d["pcs1"], d["pcs2"], atol=2e-4, rtol=2e-4, knn_graph=g)
