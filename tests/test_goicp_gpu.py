"""GPU: the Go-ICP registration (alignnet_goicp_register*, csrc/alignnet_goicp.hip) against the restatement tests/goicp_ref.py: the
evaluation kernel's per-node bounds through the debug hook, whole searches level by level, batches, rows and the refine chain.

Tolerances: a node's ub / lb are sums of at most 64 squared distances taken by differences in fp64 on both sides; what differs is the order
of the sums, the fused multiply-adds and the last bit of sin / cos / the means: 1e-9 relative is what the issue sets and three orders above
that.  An lb term whose d - gamma is within rounding of 0 contributes at most (1e-13)^2: the absolute floor 1e-18.  Per-level counts are
compared exactly; tests/test_goicp_cpu.py asserts that no decision of these cases lies within 1e-7 of its threshold."""
import numpy as np
import pytest

import alignnet3d
from tests import goicp_cases as K
from tests import goicp_ref as G
from tests.helpers import small_cfg

pytestmark = pytest.mark.gpu
KEYS = ("transforms", "error", "lower_bound", "fitness", "status", "evaluated", "survived")


@pytest.fixture(scope="module")
def eng(gpu_required):
    e = alignnet3d.Engine(small_cfg(N=64, nb=12))
    yield e
    e.close()


def _pair(ns, nq, seed, origin=(0.0, 0.0, 0.0)):
    return K.planted(ns, nq, seed, np.deg2rad(25.0 + seed), (0.1, -0.05, 0.03), noise=0.01, origin=origin)


def _nodes(depth, k, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, 1 << d, k) for d in depth], 1).astype(np.int32)


def _check_nodes(eng, s, t, depth, coords, **kw):
    pr = G.Problem(s, t, G.params(**kw))
    ub_ref, lb_ref = pr.bounds(depth, coords)
    ub, lb = eng.debug_goicp_nodes(s, t, depth, coords, **kw)
    print("ub rel err %.3g, lb abs err %.3g" % (np.abs(ub / ub_ref - 1).max(), np.abs(lb - lb_ref).max()))
    np.testing.assert_allclose(ub, ub_ref, rtol=1e-9, atol=1e-18)
    np.testing.assert_allclose(lb, lb_ref, rtol=1e-9, atol=1e-18)


NODE_KW = dict(t_half=(0.4, 0.4, 0.1), trunc=0.5, max_source=65, max_target=200)


@pytest.mark.parametrize("ns", [1, 15, 16, 17, 63, 64, 65])
@pytest.mark.parametrize("trunc", [0.5, np.inf])
def test_node_bounds_source_sizes(eng, ns, trunc):
    """|S| around the 16-row tile and the 64-lane wave; root (delta = pi) and a deep level."""
    s, t = _pair(ns, 90, ns)
    kw = dict(NODE_KW, trunc=trunc)
    _check_nodes(eng, s, t, [0, 0, 0, 0], np.zeros((1, 4), np.int32), **kw)
    _check_nodes(eng, s, t, [5, 3, 3, 2], _nodes([5, 3, 3, 2], 24, ns), **kw)


@pytest.mark.parametrize("nq", [1, 15, 16, 17, 63, 64, 65, 200])
@pytest.mark.parametrize("stage", [0, 64])
def test_node_bounds_target_sizes(eng, nq, stage):
    """|Q| around the 16-column tile and the staging chunk: stage_points = 64 puts 65 and 200 targets into two and four chunks."""
    s, t = _pair(40, nq, 100 + nq)
    kw = dict(NODE_KW, stage_points=stage)
    _check_nodes(eng, s, t, [4, 2, 2, 1], _nodes([4, 2, 2, 1], 24, nq), **kw)


def test_node_bounds_far_frame_and_subsampling(eng):
    """A frame 5 km from the origin, and clouds above max_source / max_target (the working sets are subsampled), chunked and not."""
    s, t = _pair(64, 200, 9, origin=(3000.0, -4000.0, 12.0))
    for stage in (0, 64):
        _check_nodes(eng, s, t, [4, 2, 2, 1], _nodes([4, 2, 2, 1], 24, 3), **dict(NODE_KW, stage_points=stage, trunc=np.inf))
    _check_nodes(eng, s, t, [3, 2, 2, 1], _nodes([3, 2, 2, 1], 16, 4), **dict(NODE_KW, max_source=37, max_target=111))


def test_one_pair_across_workgroups(eng):
    """One pair's nodes beyond one workgroup's share (four nodes, one per wave): 600 nodes on 150 workgroups, and 9000 nodes, where a
    workgroup walks more than one round.  Every node equals the restatement and the same node evaluated alone, bit for bit."""
    s, t = _pair(64, 200, 21)
    coords = _nodes([6, 4, 4, 2], 600, 5)
    _check_nodes(eng, s, t, [6, 4, 4, 2], coords, **NODE_KW)
    ub, lb = eng.debug_goicp_nodes(s, t, [6, 4, 4, 2], coords, **NODE_KW)
    for k in (0, 5, 599):
        u1, l1 = eng.debug_goicp_nodes(s, t, [6, 4, 4, 2], coords[k:k + 1], **NODE_KW)
        assert u1[0] == ub[k] and l1[0] == lb[k]
    s, t = _pair(16, 16, 22)
    coords = _nodes([8, 5, 5, 3], 9000, 6)
    _check_nodes(eng, s, t, [8, 5, 5, 3], coords, **NODE_KW)


def _compare(res, k, ref, origin=1.0):
    assert res["status"][k] == ref["status"], (G.STATUS_NAMES[res["status"][k]], G.STATUS_NAMES[ref["status"]])
    assert np.array_equal(res["evaluated"][k], ref["evaluated"]), (res["evaluated"][k], ref["evaluated"])
    assert np.array_equal(res["survived"][k], ref["survived"]), (res["survived"][k], ref["survived"])
    print("error %.17g ref %.17g, lower %.17g ref %.17g" % (res["error"][k], ref["error"], res["lower_bound"][k], ref["lower_bound"]))
    np.testing.assert_allclose(res["error"][k], ref["error"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(res["lower_bound"][k], ref["lower_bound"], rtol=1e-9, atol=1e-18)
    np.testing.assert_allclose(res["transforms"][k], ref["transform"], rtol=0, atol=1e-9 * origin)
    assert abs(res["fitness"][k] - ref["fitness"]) < 1e-12


@pytest.mark.parametrize("name", [n for n in K.cases() if n != "symmetric"])
def test_whole_search_matches_the_restatement(eng, name):
    """Per-level counts exactly, status, error / lower_bound to 1e-9 relative, transform to 1e-9 (times the frame's distance for the far one).
    The cases reach CERTIFIED, RESOLUTION, OVERFLOW and LEVELS (small caps), one runs the ICP starts, one is 5 km out."""
    s, t, kw = K.cases()[name]
    res = eng.goicp_register([s], [t], **kw)
    _compare(res, 0, K.reference(name), origin=5000.0 if name == "far5km" else 1.0)


def test_symmetric_cloud_error_and_certificate(eng):
    """Every optimum comes twice: which of the two poses wins is a tie, so only the error and the certificate are compared."""
    s, t, kw = K.cases()["symmetric"]
    res, ref = eng.goicp_register([s], [t], **kw), K.reference("symmetric")
    np.testing.assert_allclose(res["error"][0], ref["error"], rtol=1e-9)
    np.testing.assert_allclose(res["lower_bound"][0], ref["lower_bound"], rtol=1e-9, atol=1e-18)
    assert res["status"][0] == ref["status"]


def _batch():
    kw = dict(K.COARSER)
    names = ("noisy", "overflow", "symmetric", "starts_z")
    src = [K.cases()[n][0] for n in names]
    tgt = [K.cases()[n][1] for n in names]
    empty = np.zeros((0, 3), np.float32)
    src = src[:2] + [empty] + src[2:] + [src[0]]
    tgt = tgt[:2] + [tgt[0]] + tgt[2:] + [empty]
    return src, tgt, kw


@pytest.mark.parametrize("starts", [0, 3])
def test_heterogeneous_batch_equals_pairs_alone(eng, starts):
    """Pairs of different sizes, an empty source and an empty target in one call: each pair bit-identical to the pair alone and to a second
    call; the empty ones are EMPTY with the identity and error 0."""
    src, tgt, kw = _batch()
    kw = dict(kw, starts=starts, start_radius=0.3)
    res = eng.goicp_register(src, tgt, **kw)
    again = eng.goicp_register(src, tgt, **kw)
    for key in KEYS:
        assert np.array_equal(res[key], again[key]), key
    for k in range(len(src)):
        one = eng.goicp_register([src[k]], [tgt[k]], **kw)
        for key in KEYS:
            assert np.array_equal(res[key][k], one[key][0]), (k, key)
    for k in (2, len(src) - 1):
        assert res["status"][k] == G.EMPTY and res["error"][k] == 0.0 and np.array_equal(res["transforms"][k], np.eye(4))
        assert res["evaluated"][k].sum() == 0
    if starts == 0:
        _compare(res, 0, G.search(src[0], tgt[0], G.params(**kw)))


def test_batch_in_several_chunks(eng):
    """max_frontier = 2^22 makes a pair's buffers 192 MiB: seven pairs take two chunks of the 1 GiB budget.  Same results as alone."""
    src, tgt, kw = _batch()
    src, tgt = src + src[:1], tgt + tgt[:1]
    kw = dict(kw, max_frontier=1 << 22)
    res = eng.goicp_register(src, tgt, **kw)
    for k in (0, 3, 5, 6):
        one = eng.goicp_register([src[k]], [tgt[k]], **dict(kw, max_frontier=1 << 16))
        for key in KEYS:
            assert np.array_equal(res[key][k], one[key][0]), (k, key)


def test_rows_equal_host_arrays(eng):
    src, tgt, kw = _batch()
    off = np.zeros((len(src) + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(x) for x in src]); off[1:, 1] = np.cumsum([len(x) for x in tgt])
    eng.upload_dataset(np.concatenate(src, 0), np.concatenate(tgt, 0), off, np.zeros((len(src), 12), np.float32))
    rows = [4, 0, 2, 1, 4]
    a = eng.goicp_register_rows(rows, **kw)
    b = eng.goicp_register([src[r] for r in rows], [tgt[r] for r in rows], **kw)
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
    ar = eng.goicp_register_rows(rows, refine="p2p", **kw)
    br = eng.icp_refine_rows(rows, a["transforms"], radius=0.10, its=30)
    assert np.array_equal(ar["transforms"], br["transforms"]) and np.array_equal(ar["search_transforms"], a["transforms"])


def test_refine_chain(eng):
    """refine="p2p" = icp_refine on the FULL clouds (radius 0.10, 30 iterations) started from the search's transform."""
    s, t, kw = K.cases()["planted170"]
    plain = eng.goicp_register([s], [t], **kw)
    res = eng.goicp_register([s], [t], refine="p2p", **kw)
    assert np.array_equal(res["search_transforms"], plain["transforms"]) and np.array_equal(res["error"], plain["error"])
    ref = eng.icp_refine([s], [t], plain["transforms"], radius=0.10, its=30)
    for key in ("transforms", "fitness", "rmse", "iterations"):
        assert np.array_equal(res[key], ref[key]), key
    yaw = np.arctan2(res["transforms"][0, 1, 0], res["transforms"][0, 0, 0])
    assert abs((yaw - K.YAW_170 + np.pi) % (2 * np.pi) - np.pi) < np.deg2rad(1.0)


def test_entry_errors(eng):
    s, t, kw = K.cases()["levels"]
    with pytest.raises(NotImplementedError):
        eng.goicp_register([s], [t], constrained=False, **kw)
    for bad in (dict(yaw_res=0.0), dict(max_levels=25), dict(stage_points=40), dict(max_frontier=0), dict(trunc=0.0), dict(yaw_half=4.0)):
        with pytest.raises(alignnet3d.EngineError):
            eng.goicp_register([s], [t], **dict(kw, **bad))
    res = eng.goicp_register([s], [t], **kw)   # the engine still works
    assert res["status"][0] == G.LEVELS
