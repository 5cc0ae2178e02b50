"""NumPy restatement of knn_kernel's select (alignnet-3d_amd/csrc/kernels_dgcnn.h), used ONLY to prove what the test inputs reach (which of the three
select paths a query takes) and to show on the CPU that a wrong select would be caught.  The kernel's result is always judged against the fp64 oracle
(R.knn_indices), never against this file.

Restated: the centroid (centroid_body's summation order), the fp32 distance expression, lane = index & 63, the k-th smallest lane minimum on the upper 16
key bits, the survivor count M and the path it selects (4a: M <= 64, 4b: M <= 128, 4c: more), and the rows each path emits.  fmaf is emulated through
float64 (the product is exact there, the sum is rounded twice), so a survivor exactly on the bound may fall the other way: the proofs assert counts, not
membership.

check_rows() is the judgement both the CPU proofs and the GPU tests apply to a neighbour table."""
import numpy as np

from oracle import alignnet_ref as R
from tests.sampler_cases import copy_classes

K = 20
F32 = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def centroid(pc):
    """centroid_body (kernels_infer.h): 256 threads stride over the points, a butterfly per wave, the four wave sums left to right, / N -- all fp32."""
    N = len(pc)
    s = np.zeros((256, 3), F32)
    for lo in range(0, N, 256):
        c = pc[lo:lo + 256]
        s[:len(c)] += c
    v = s.reshape(4, 64, 3)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, np.arange(64) ^ o]
    red = v[:, 0]
    return (((red[0] + red[1]) + red[2]) + red[3]) / F32(N)


def fkey(d):
    b = np.ascontiguousarray(d, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def distances(x, q):
    """d[i, j] of the queries x[q] to every candidate, as the kernel rounds it: pp = fma(z, z, fma(y, y, x x)); inner = fma(-2 qz, z, fma(-2 qy, y, (-2 qx) x));
    d = (qq + inner) + pp."""
    pp = _fma(x[:, 2], x[:, 2], _fma(x[:, 1], x[:, 1], x[:, 0] * x[:, 0]))
    q2 = F32(-2.0) * x[q]
    inner = _fma(q2[:, 2:3], x[None, :, 2], _fma(q2[:, 1:2], x[None, :, 1], q2[:, 0:1] * x[None, :, 0]))
    return (pp[q][:, None] + inner) + pp[None, :]


def slots_per_lane(N):
    return 16 if N <= 1024 else 32 if N <= 2048 else 64


def queries_per_workgroup(B, N):
    """launch_knn's grid rule: 256 queries per workgroup, halved (down to 32) while the grid has fewer than 512 workgroups."""
    qpw = 256
    while qpw > 32 and 2 * B * ((N + qpw - 1) // qpw) < 512:
        qpw >>= 1
    return qpw


def select(pc, k=K, rows=True, mutate=None, chunk=512):
    """pc [N, 3] float32 (raw cloud).  Returns (M [N] survivors of the first bound, path [N] of "a" / "b" / "c", rows [N, k] or None).
    mutate: None, or a WRONG kernel -- "c_no_lt_pass": 4c emits the first k candidates <= T in index order (no pass for those strictly below T);
    "b_list_64": 4b sees only the first 64 entries of its list."""
    pc = np.ascontiguousarray(pc, F32)
    N = len(pc)
    per = slots_per_lane(N)
    x = pc - centroid(pc)
    M = np.zeros(N, np.int64)
    out = np.zeros((N, k), np.int64) if rows else None
    for lo in range(0, N, chunk):
        q = np.arange(lo, min(N, lo + chunk))
        d = distances(x, q)
        pad = np.full((len(q), per * 64), np.inf, F32)
        pad[:, :N] = d
        lmin16 = fkey(pad.reshape(len(q), per, 64).min(axis=1)) >> np.uint32(16)
        kth = np.sort(lmin16, axis=1)[:, k - 1].astype(np.uint32)
        T0 = np.minimum((kth << np.uint32(16)) | np.uint32(0xffff), np.uint32(0xff7fffff))
        key = fkey(d)
        surv = key <= T0[:, None]
        M[q] = surv.sum(1)
        if not rows:
            continue
        for i, qi in enumerate(q):
            m = M[qi]
            if m <= 64:                                   # 4a: rank by (key, index), nearest first
                idx = np.flatnonzero(surv[i])
                out[qi] = idx[np.lexsort((idx, key[i, idx]))[:k]]
            elif m <= 128:                                # 4b: bisect the list, emit in index order: below T, then equal to T
                idx = np.flatnonzero(surv[i])
                if mutate == "b_list_64":
                    idx = idx[:64]
                kk = key[i, idx]
                T = np.sort(kk)[k - 1]
                out[qi] = np.concatenate([idx[kk < T], idx[kk == T]])[:k]
            else:                                         # 4c: bisect all candidates (float compares), emit in index order
                T = np.sort(d[i])[k - 1]
                if mutate == "c_no_lt_pass":
                    out[qi] = np.flatnonzero(d[i] <= T)[:k]
                else:
                    out[qi] = np.concatenate([np.flatnonzero(d[i] < T), np.flatnonzero(d[i] == T)])[:k]
    path = np.where(M <= 64, "a", np.where(M <= 128, "b", "c"))
    return M, path, out


def oracle(pc, k=K):
    """The fp64 oracle on the mean-centred cloud: (want [N, k] = R.knn_indices' selection as a set in index order, dist [N, N], eps [N, 1] = the
    fp32 rounding of the distance formula, 64 eps32 (|q|^2 + max |x|^2), the margin of tests/test_forward_gpu.py::test_knn_graph_against_oracle, kth [N, 1] = the
    distance at rank k)."""
    x = np.asarray(pc, np.float64)
    x = x - x.mean(axis=0, keepdims=True)
    sq = (x * x).sum(-1)
    # R.knn_indices' expression (utils/tf_util_dgcnn.py:638-671) with the inner product written out per element: through BLAS, `x @ x.T` rounds the
    # products of bit-identical rows differently from block to block (1e-16), and the stable sort then orders exact copies by that noise, not by index
    inner = x[:, None, 0] * x[None, :, 0] + x[:, None, 1] * x[None, :, 1] + x[:, None, 2] * x[None, :, 2]
    dist = sq[:, None] - 2.0 * inner + sq[None, :]
    # the k smallest with ties to the lower index (what the stable sort selects), without sorting N^2 entries: everything below the k-th value, then
    # the lowest indices among those equal to it
    kth = np.partition(dist, k - 1, axis=1)[:, k - 1:k]
    below, equal = dist < kth, dist == kth
    take = below | (equal & (np.cumsum(equal, axis=1) <= k - below.sum(1, keepdims=True)))
    want = np.nonzero(take)[1].reshape(len(x), k)                      # as a set, in index order
    if len(x) <= 256:   # ... and it is R.knn_indices' selection: the distances of its rows are those of `want`, to fp64 rounding
        ref = R.knn_indices(x[None], k)[0]
        assert np.abs(np.sort(np.take_along_axis(dist, ref, axis=1), axis=1) - np.sort(np.take_along_axis(dist, want, axis=1), axis=1)).max() <= 1e-12 * max(1.0, sq.max())
    eps = 64 * np.finfo(np.float32).eps * (sq[:, None] + sq.max())
    return want, dist, eps, kth


def undecided(pc, k=K, orc=None):
    """[N] bool: another unique point's fp64 distance lies within 2 x eps of the distance of the group that holds rank k -- fp32 cannot be asked to
    agree with fp64 on such a query.  Exact copies never make a query undecided: both sides break those ties by index."""
    want, dist, eps, dk = orc if orc is not None else oracle(pc, k)
    first, _ = copy_classes(pc)
    reps = np.unique(first)
    return (np.abs(dist[:, reps] - dk) <= 2 * eps).sum(1) > 1     # (the rank-k group itself counts once)


def check_rows(got, pc, k=K, path=None, orc=None):
    """The judgement of a neighbour table got [N, k] of the cloud pc [N, 3] (raises AssertionError).  For every query: k distinct in-range indices; nothing
    nearer left out (up to eps); nearest first where `path` says 4a (4b / 4c emit in index order: include/alignnet_hip.h); within the tie group at rank k
    the listed copies are the group's lowest indices; and every decided row equals the oracle's as a set.  Returns the number of undecided queries."""
    got = np.asarray(got, np.int64)
    N = len(pc)
    orc = orc if orc is not None else oracle(pc, k)
    want, dist, eps, kth = orc
    assert got.shape == (N, k) and got.min() >= 0 and got.max() < N, "index out of range"
    srt = np.sort(got, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "duplicate neighbour"
    dg = np.take_along_axis(dist, got, axis=1)
    assert (dg <= kth + eps).all(), "a listed neighbour is farther than the k-th nearest"
    if path is not None:
        a = np.asarray(path) == "a"
        assert (np.diff(dg[a], axis=1) >= -eps[a]).all(), "4a row not nearest-first"
        # 4b / 4c: two runs, each in index order -- the candidates strictly nearer than the rank-k distance, then the tie group at rank k
        bc = ~a & ~undecided(pc, k, orc)
        run = (dg[bc] >= kth[bc] - 2 * eps[bc]).astype(np.int64) * N + got[bc]
        assert (np.diff(run, axis=1) > 0).all(), "4b / 4c row not in (nearer, then ties at rank k) x index order"
    # the tie group at rank k = the copy class of the farthest listed neighbour: its listed members must be its lowest indices
    first, _ = copy_classes(pc)
    order = np.lexsort((np.arange(N), first))
    rank_in_class = np.empty(N, np.int64)
    rank_in_class[order] = np.arange(N) - np.searchsorted(first[order], first[order], side="left")
    far = np.take_along_axis(got, dg.argmax(axis=1)[:, None], axis=1)
    member = first[got] == first[far]
    worst = np.where(member, rank_in_class[got], -1).max(axis=1)
    und = undecided(pc, k, orc)
    bad = (worst != member.sum(1) - 1) & ~und
    assert not bad.any(), "%d queries list copies of the rank-k point that are not its lowest indices (e.g. query %d)" % (int(bad.sum()), int(np.argmax(bad)))
    differ = (srt != want).any(axis=1) & ~und
    assert not differ.any(), "%d decided rows differ from the fp64 oracle's as sets (e.g. query %d: %s, oracle %s)" % (
        int(differ.sum()), int(np.argmax(differ)), srt[np.argmax(differ)].tolist(), want[np.argmax(differ)].tolist())
    return int(und.sum())
