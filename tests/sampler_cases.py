"""Clouds as the batch sampler draws them (provider.py:97-98 `np.random.choice(n, N, replace=True)`, alignnet_dataset_sample): every batch is
resampled WITH replacement, so a real batch holds bit-identical copies of points -- a far car of 7 returns becomes N points of N / 7
copies each, an empty cloud N points at the origin.  The other network tests draw R.synth_pairs (N distinct points).

A toy dataset whose clouds have 0, 1, 2, 7, 12, 19, 21, 24, 60 and 300 unique points, and one larger than any N used; every cloud is
the head of an R.synth_pairs(1, n) pair (car-sized, 4 - 20 m from the origin, labels of that pair).  Batches come from
oracle/dataset_ref.sample_batch without jitter, which tests/test_dataset_gpu.py holds bit-exact to the device sampler.

Three more rows per kNN size hold clouds whose SOURCE lists a point several times (`weighted`): the sampler then draws unequal
multiplicities -- a point A with about 10 copies next to its nearest neighbour B with about 90 (or nearly all the rest) -- which is the
only way a uniform draw puts a query on the kNN kernel's 4b / 4c select paths while the group that holds rank k is not the nearest one.

Also here: the copy classes of a cloud and the checkers of the "first copy wins" rule of the max-pools (shared by the CPU proofs and the
GPU tests)."""
import functools

import numpy as np

from oracle import alignnet_ref as R
from oracle import dataset_ref as D

BIG = 2500                                        # larger than every N the tests sample to
UNIQUE = (0, 1, 2, 7, 12, 19, 21, 24, 60, 300, BIG)
# (unique points of tower 1, of tower 2) per dataset row
ROWS = [(0, 12), (1, 2), (7, 19), (21, 24), (60, 300), (300, 0), (0, 0), (BIG, 7),
        (12, 1), (19, 60), (24, 21), (2, BIG), (300, 12), (7, 1), (60, 19), (24, 2)]
MIXED = list(range(8))                            # one empty tower (either side), both empty, tiny, about 300, larger than N: all kinds in one batch
ONE_EMPTY_TOWER = [0, 5]
BOTH_EMPTY = [6]
KNN_SIZES = (200, 1100, 2100)                     # knn_kernel<16> / <32> / <64>: N <= 1024 / 2048 / 4096
WEIGHTED_ROW = {N: len(ROWS) + i for i, N in enumerate(KNN_SIZES)}     # tower 1: A x 1, B x 9, the rest once; tower 2: A x 1, B x (S - 4), three others


def knn_rows(N):
    """Dataset rows of the kNN cases at cloud size N: every row at the smallest size; at the larger ones every kind of cloud once (the fp64 oracle is N^2
    per cloud), each with the weighted-source row of that size."""
    return (list(range(len(ROWS))) if N == KNN_SIZES[0] else MIXED + [8, 9, 10]) + [WEIGHTED_ROW[N]]


TOWER2_EMPTY = [len(ROWS) + len(KNN_SIZES) + i for i in range(6)]      # every cloud of tower 2 empty
_TOWER2_EMPTY_COUNTS = (7, 19, 60, 300, 24, 12)
SEED = 20


def _label_row(d):
    return np.concatenate([d[k][0] for k in ("translations", "rel_angles", "pc1_centers", "pc2_centers", "pc1_angles", "pc2_angles")]).astype(np.float32)


def weighted_sources(N, seed):
    """Two source clouds of S = N // 10 entries (a draw of N gives about 10 copies per entry) from one synth cloud of S points: A = its point 0, B = A's
    nearest neighbour.  "b": [A, B x 9, S - 10 others] -- a query in A has about 10 own copies, rank k = 20 falls into B's about 90 (select path 4b);
    "c": [A, B x (S - 4), 3 others] -- B holds nearly all of the cloud (path 4c)."""
    S = N // 10
    d = R.synth_pairs(1, S, seed=seed, dtype=np.float32)
    out = []
    for key, kind in (("pcs1", "b"), ("pcs2", "c")):
        p = d[key][0]
        dist = ((p.astype(np.float64) - p[0].astype(np.float64)) ** 2).sum(1)
        dist[0] = np.inf
        nb = int(np.argmin(dist))
        others = [i for i in range(1, S) if i != nb]
        order = [0] + [nb] * 9 + others[:S - 10] if kind == "b" else [0] + [nb] * (S - 4) + others[:3]
        assert len(order) == S
        out.append(p[order])
    return out[0], out[1], _label_row(d)


@functools.lru_cache(maxsize=None)
def dataset():
    """(points1, points2), offsets [rows + 1, 2], labels [rows, 12] in the layout of Engine.upload_dataset / oracle.dataset_ref.sample_batch."""
    p1, p2, lab = [], [], []
    counts = list(ROWS) + [None] * len(KNN_SIZES) + [(c, 0) for c in _TOWER2_EMPTY_COUNTS]
    for row, c in enumerate(counts):
        if c is None:
            a, b, l = weighted_sources(KNN_SIZES[row - len(ROWS)], SEED + row)
        else:
            d = R.synth_pairs(1, max(c[0], c[1], 1), seed=SEED + row, dtype=np.float32)
            a, b, l = d["pcs1"][0][:c[0]], d["pcs2"][0][:c[1]], _label_row(d)
        p1.append(a); p2.append(b); lab.append(l)
    off = np.zeros((len(counts) + 1, 2), np.int64)
    off[1:, 0] = np.cumsum([len(a) for a in p1])
    off[1:, 1] = np.cumsum([len(b) for b in p2])
    return (np.concatenate(p1).astype(np.float32), np.concatenate(p2).astype(np.float32)), off, np.stack(lab)


def batch(rows, N, seed=77):
    """The batch the device sampler draws for `rows` (no jitter): dict with pcs1, pcs2 [B, N, 3] float32 and the six label arrays, as R.synth_pairs returns."""
    pts, off, lab = dataset()
    a, b, labs, _ = D.sample_batch(pts, off, lab, list(rows), N, seed)
    d = dict(labs)
    d["pcs1"], d["pcs2"] = a, b
    return d


def unique_points(rows, tower):
    """Unique points of the SOURCE clouds of `rows` (the draw may miss some)."""
    pts, off, _ = dataset()
    return [len(np.unique(pts[tower][off[r, tower]:off[r + 1, tower]].view(np.uint32).reshape(-1, 3), axis=0)) for r in rows]


def copy_classes(pc):
    """pc [N, 3] float32 -> (first [N]: lowest index holding the same BITS as point i, count [N]: copies of point i, itself included)."""
    bits = np.ascontiguousarray(pc, np.float32).view(np.uint32).reshape(-1, 3)
    _, first_of, inv, cnt = np.unique(bits, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    return first_of[inv], cnt[inv]


# ---- the max-pools' "first maximum wins" on copies (kernels_train_fwd.h, kernels_train_generic.h, kernels_train_dgcnn.h) ----
# A rigid motion applied to every point of a cloud alike keeps bit-copies bit-copies, so the copy classes of the raw batch are those of every stage's frame;
# copies have identical features (and, with the dgcnn backbone, identical neighbour rows), so in every channel all copies of the winner tie exactly.
def check_pool_first_copy(pool, pcs):
    """pool [2, B, C]: arg-max point per cloud and channel (ALIGNNET_DECISION_POOL_POINT); pcs = (pcs1, pcs2).  Exact: no point of index below the winner is a
    bit-copy of it.  Returns copies-of-the-winner [2, B, C]."""
    ncopies = np.zeros(pool.shape, np.int64)
    for t in range(2):
        for b in range(pool.shape[1]):
            first, cnt = copy_classes(pcs[t][b])
            w = pool[t, b]
            bad = first[w] != w
            assert not bad.any(), "tower %d cloud %d: %d pool winners are not the first copy of their point (e.g. channel %d: point %d is a copy of point %d)" % (
                t, b, int(bad.sum()), int(np.argmax(bad)), int(w[np.argmax(bad)]), int(first[w[np.argmax(bad)]]))
            ncopies[t, b] = cnt[w]
    return ncopies


def check_slot_first_copy(slot, graph, pcs):
    """slot [2, B, N, C]: arg-max neighbour slot per point and channel (ALIGNNET_DECISION_EDGE_SLOT); graph [2, B, N, k] the step's neighbour table.  Exact: no
    earlier slot of the row holds a copy of the point in the winning slot.  Returns slots-holding-a-copy-of-the-winner [2, B, N, C]."""
    ncopies = np.zeros(slot.shape, np.int64)
    for t in range(2):
        for b in range(slot.shape[1]):
            first, _ = copy_classes(pcs[t][b])
            cls = first[graph[t, b]]                                   # [N, k] copy class of every slot
            same = cls[:, :, None] == cls[:, None, :]                  # [N, k, k]
            first_slot = same.argmax(axis=2)                           # lowest slot of the row holding that class
            s = slot[t, b]
            bad = np.take_along_axis(first_slot, s, axis=1) != s
            assert not bad.any(), "tower %d cloud %d: %d slot winners have a copy of their neighbour in an earlier slot" % (t, b, int(bad.sum()))
            ncopies[t, b] = np.take_along_axis(same.sum(axis=2), s, axis=1)
    return ncopies
