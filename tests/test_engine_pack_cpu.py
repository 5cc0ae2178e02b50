"""CPU: the packing helpers of alignnet3d/engine.py's registration section -- _pack_pairs (lists of clouds -> two float32 blobs and the [B + 1, 2]
offsets table every host entry point takes) and _one_pair (the one pair of the debug_* hooks) -- against the blocks the callers used to carry, kept
here word for word.  No device, no library call."""
import numpy as np
import pytest

from alignnet3d.engine import _one_pair, _pack_pairs


def _pasted_pack(sources, targets):
    """the block as icp_refine, evaluate_registration, register, ... each held it"""
    B = len(sources)
    off = np.zeros((B + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(s) for s in sources]); off[1:, 1] = np.cumsum([len(t) for t in targets])
    cat = lambda L: np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32).reshape(-1, 3) for x in L], 0)) if L else np.zeros((0, 3), np.float32)
    p1, p2 = cat(sources), cat(targets)
    return p1, p2, off


def _pasted_one(source, target, T):
    """the block as the debug_icp_* hooks each held it"""
    p1 = np.ascontiguousarray(np.asarray(source, np.float32).reshape(-1, 3)); p2 = np.ascontiguousarray(np.asarray(target, np.float32).reshape(-1, 3))
    Tm = np.ascontiguousarray(np.asarray(T, np.float64).reshape(16))
    return p1, p2, Tm


def _cloud(rng, n, dtype=np.float32):
    return rng.standard_normal((n, 3)).astype(dtype)


def _check_blob(a, want):
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 3 and a.flags["C_CONTIGUOUS"]
    assert a.shape == want.shape and np.array_equal(a, want)


def _cases():
    rng = np.random.default_rng(7)
    wide = rng.standard_normal((9, 6))                      # float64; its [:, :3] and [::2, :3] views are not contiguous
    fort = np.asfortranarray(rng.standard_normal((4, 3)))   # float64, column-major
    return {
        "empty_list": ([], []),
        "empty_pair": ([np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.float32)]),
        "float64_strided": ([wide[:, :3], wide[::2, 3:], fort], [fort, wide[1::3, :3], wide[:, 3:]]),
        "sizes_0_1_3_vs_2_0_5": ([_cloud(rng, n) for n in (0, 1, 3)], [_cloud(rng, n) for n in (2, 0, 5)]),
        "lists_and_ints": ([[[1, 2, 3]], np.arange(6).reshape(2, 3)], [[[0.5, 0.25, 0.125], [4, 5, 6]], np.arange(9, dtype=np.int64).reshape(3, 3)]),
    }


@pytest.mark.parametrize("name", sorted(_cases()))
def test_pack_pairs(name):
    sources, targets = _cases()[name]
    p1, p2, off = _pack_pairs(sources, targets)
    w1, w2, woff = _pasted_pack(sources, targets)
    _check_blob(p1, w1)
    _check_blob(p2, w2)
    B = len(sources)
    assert off.dtype == np.int64 and off.shape == (B + 1, 2) and off.flags["C_CONTIGUOUS"] and np.array_equal(off, woff)
    # the table stated on its own: row 0 is zero, the differences are the clouds' point counts, the last row is the blobs' lengths
    n1 = [np.asarray(s).size // 3 for s in sources]
    n2 = [np.asarray(t).size // 3 for t in targets]
    assert off[0].tolist() == [0, 0]
    assert np.diff(off[:, 0]).tolist() == [len(s) for s in sources] and np.diff(off[:, 1]).tolist() == [len(t) for t in targets]
    assert off[-1].tolist() == [sum(n1), sum(n2)] == [len(p1), len(p2)]
    for b in range(B):
        assert np.array_equal(p1[off[b, 0]:off[b + 1, 0]], np.asarray(sources[b], np.float32).reshape(-1, 3))
        assert np.array_equal(p2[off[b, 1]:off[b + 1, 1]], np.asarray(targets[b], np.float32).reshape(-1, 3))


def test_pack_pairs_values_by_hand():
    p1, p2, off = _pack_pairs([np.zeros((0, 3)), [[1, 2, 3]], np.arange(9.0).reshape(3, 3)], [np.ones((2, 3)), np.zeros((0, 3)), np.full((5, 3), 2.5)])
    assert off.tolist() == [[0, 0], [0, 2], [1, 2], [4, 7]]
    assert p1.tolist() == [[1, 2, 3], [0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert p2.tolist() == [[1, 1, 1]] * 2 + [[2.5, 2.5, 2.5]] * 5
    e1, e2, eoff = _pack_pairs([], [])
    assert e1.shape == e2.shape == (0, 3) and e1.dtype == e2.dtype == np.float32 and eoff.tolist() == [[0, 0]]


def test_pack_pairs_copies():
    src = [np.arange(6, dtype=np.float32).reshape(2, 3)]
    p1, _, _ = _pack_pairs(src, src)
    p1[:] = -1.0
    assert src[0][0, 0] == 0.0   # the blob is the call's own


@pytest.mark.parametrize("name", sorted(_cases()))
def test_one_pair(name):
    sources, targets = _cases()[name]
    rng = np.random.default_rng(11)
    T64 = rng.standard_normal((4, 4))
    for source, target in zip(sources or [np.zeros((0, 3))], targets or [np.zeros((0, 3))]):
        for T in (T64, T64.T, T64.astype(np.float32), T64.reshape(16).tolist()):   # contiguous, transposed view, float32, a list
            got, want = _one_pair(source, target, T), _pasted_one(source, target, T)
            _check_blob(got[0], want[0])
            _check_blob(got[1], want[1])
            assert got[2].dtype == np.float64 and got[2].shape == (16,) and got[2].flags["C_CONTIGUOUS"] and np.array_equal(got[2], want[2])
    assert np.array_equal(_one_pair(np.zeros((0, 3)), np.zeros((0, 3)), T64.T)[2], T64.T.reshape(16))   # row-major of the view, not of its memory


def test_one_pair_without_transform():
    p1, p2, Tm = _one_pair(np.zeros((2, 3)), [[1, 2, 3]], None)   # the hooks of the global methods carry no transform
    assert p1.shape == (2, 3) and p2.tolist() == [[1, 2, 3]] and Tm is None
