"""CPU proofs about the inputs of tests/test_sampler_clouds_gpu.py (tests/sampler_cases.py), through the NumPy restatement of knn_kernel's select
(tests/knn_select_ref.py):
  * coverage: for each compiled instantiation of knn_kernel the chosen clouds put at least 100 queries on each select path 4a / 4b / 4c, and some
    queries on 4b and on 4c whose rank-k group is not the nearest one (the only ones on which those paths emit from two passes);
  * the cap on queries fp32 cannot decide (clouds of at most 60 unique points: at most 1e-3 of a case's queries);
  * the restated select passes the judgement the GPU test applies (check_rows), and three WRONG kernels restated here fail it on these inputs while the
    inputs of the present kNN tests cannot tell them from the right one: 4c without its `< T` pass, 4b's list cut at 64, a pool winner taken as the last
    equal maximum."""
import numpy as np
import pytest

from oracle import alignnet_ref as R
from tests import knn_select_ref as KS
from tests import sampler_cases as SC

K = KS.K


@pytest.fixture(scope="module", params=SC.KNN_SIZES)
def restated(request):
    """The restated select on every cloud of the kNN cases at one size (computed once per size): list of (row, tower, unique points, cloud, M, path, rows)."""
    N = request.param
    rows = SC.knn_rows(N)
    d = SC.batch(rows, N)
    out = []
    for t, key in enumerate(("pcs1", "pcs2")):
        uniq = SC.unique_points(rows, t)
        for b, row in enumerate(rows):
            M, path, got = KS.select(d[key][b])
            out.append((row, t, uniq[b], d[key][b], M, path, got))
    return N, out


def test_every_select_path_is_reached(restated):
    N, clouds = restated
    count = {p: sum(int((path == p).sum()) for *_, path, _ in clouds) for p in "abc"}
    # queries on 4b / 4c whose own copies are fewer than k: rank k lies in a farther group, both passes (`< T`, then `== T`) emit
    two_pass = {p: 0 for p in "bc"}
    for row, t, u, pc, M, path, got in clouds:
        _, cnt = SC.copy_classes(pc)
        for p in "bc":
            two_pass[p] += int(((path == p) & (cnt < K)).sum())
    print("knn_kernel<%d> N=%d: queries per path %s, of them with rank k outside the nearest group %s" % (KS.slots_per_lane(N), N, count, two_pass))
    assert all(c >= 100 for c in count.values()), count
    assert all(c >= 3 for c in two_pass.values()), two_pass
    # the all-zero cloud: every candidate survives
    zero = [M for row, t, u, pc, M, path, got in clouds if u == 0]
    assert zero and all((M == N).all() for M in zero)


def test_restated_select_passes_the_judgement_and_undecided_cap(restated):
    N, clouds = restated
    for row, t, u, pc, M, path, got in clouds:
        und = KS.check_rows(got, pc, path=path)
        if u <= 60:
            assert und <= 1e-3 * N, (row, t, u, und)
        if u == 0:
            np.testing.assert_array_equal(got, np.tile(np.arange(K), (N, 1)))
        print("N=%d row %d tower %d: %d unique points, undecided queries %d" % (N, row, t, u, und))


@pytest.mark.parametrize("mutate,path", [("c_no_lt_pass", "c"), ("b_list_64", "b")])
def test_wrong_select_is_caught(mutate, path):
    """The wrong kernel differs from the right one on some query of the weighted-source clouds, and check_rows refuses its table."""
    N = SC.KNN_SIZES[0]
    d = SC.batch([SC.WEIGHTED_ROW[N]], N)
    pc = d["pcs1" if path == "b" else "pcs2"][0]
    _, p, right = KS.select(pc)
    _, _, wrong = KS.select(pc, mutate=mutate)
    assert (wrong != right).any(axis=1).sum() >= 3 and (p[(wrong != right).any(axis=1)] == path).all()
    KS.check_rows(right, pc, path=p)
    with pytest.raises(AssertionError, match="differ from the fp64 oracle|index order"):
        KS.check_rows(wrong, pc, path=p)


def test_present_knn_inputs_never_leave_4a():
    """The inputs of tests/test_forward_gpu.py::test_knn_graph_against_oracle and ::test_knn_graph_ties_bit_exact (the 13^3 lattice included): no query has
    more than 64 survivors, so those tests run neither 4b nor 4c and cannot tell the wrong kernels above from the right one."""
    worst = 0
    for N, B in [(20, 2), (64, 3), (200, 3), (1024, 2), (1500, 2), (2048, 1), (3000, 1), (4096, 2)]:
        d = R.synth_pairs(B, N, seed=77 + N, dtype=np.float32)
        for pcs in (d["pcs1"], d["pcs2"]):
            for b in range(B if N <= 2048 else 1):      # (the largest sizes: one cloud per tower keeps this test at seconds)
                worst = max(worst, int(KS.select(pcs[b], rows=False)[0].max()))
    for N in (64, 1536, 4096):
        rng = np.random.default_rng(5 + N)
        half = rng.integers(-6, 7, size=(2, N // 2, 3)).astype(np.float32)
        pcs = np.concatenate([half, -half], axis=1)
        pcs = pcs[:, rng.permutation(N)]
        for b in range(2):
            worst = max(worst, int(KS.select(pcs[b], rows=False)[0].max()))
    print("largest survivor count on the present kNN tests' inputs:", worst)
    assert worst <= 64


def test_last_equal_maximum_is_caught():
    """A pool that takes the LAST of equal maxima: refused by the first-copy rule on a sampler batch; on distinct points (R.synth_pairs, the other tests'
    input) the rule has nothing to refuse -- there are no copies."""
    rng = np.random.default_rng(3)
    W = rng.normal(size=(3, 24)).astype(np.float32)
    d = SC.batch(SC.MIXED, 128)
    pcs = (d["pcs1"], d["pcs2"])
    feat = [p @ W for p in pcs]                                           # copies of a point have identical features: exact ties in every channel
    first = np.stack([f.argmax(axis=1) for f in feat])                    # [2, B, C] first maximum
    last = np.stack([f.shape[1] - 1 - f[:, ::-1].argmax(axis=1) for f in feat])
    copies = SC.check_pool_first_copy(first, pcs)
    assert (copies > 1).mean() > 0.5
    with pytest.raises(AssertionError, match="not the first copy"):
        SC.check_pool_first_copy(last, pcs)
    s = R.synth_pairs(len(SC.MIXED), 128, dtype=np.float32)
    spcs = (s["pcs1"], s["pcs2"])
    sfeat = [p @ W for p in spcs]
    slast = np.stack([f.shape[1] - 1 - f[:, ::-1].argmax(axis=1) for f in sfeat])
    assert (SC.check_pool_first_copy(slast, spcs) == 1).all()
    # the same for the max over the k neighbour slots
    graph = np.stack([np.stack([R.knn_indices(p[b:b + 1].astype(np.float64), K)[0] for b in range(len(p))]) for p in pcs])   # [2, B, N, k]
    edge = [np.take_along_axis(f[:, None], g[..., None], axis=2) for f, g in zip(feat, graph)]                                # [B, N, k, C]
    sfirst = np.stack([e.argmax(axis=2) for e in edge])
    slast = np.stack([K - 1 - e[:, :, ::-1].argmax(axis=2) for e in edge])
    assert (SC.check_slot_first_copy(sfirst, graph, pcs) > 1).mean() > 0.5
    with pytest.raises(AssertionError, match="earlier slot"):
        SC.check_slot_first_copy(slast, graph, pcs)


def test_inputs_hold_what_the_issue_lists():
    pts, off, lab = SC.dataset()
    have = set()
    for t in range(2):
        have |= set(SC.unique_points(range(len(SC.ROWS)), t))
    assert have == set(SC.UNIQUE)
    d = SC.batch(SC.MIXED, 128)
    assert not d["pcs1"][0].any() and not d["pcs2"][5].any() and not d["pcs1"][6].any() and not d["pcs2"][6].any()
    first, cnt = SC.copy_classes(d["pcs2"][7])                            # 7 returns -> 128 points
    assert len(np.unique(first)) <= 7 and cnt.min() >= 2
    e = SC.batch(SC.TOWER2_EMPTY, 128)
    assert not e["pcs2"].any() and all(p.any() for p in e["pcs1"])
