"""numpy restatement of the k-NN graph and its consumers (goi_knn_graph, goi_knn_majority, goi_hyperplane_amd.knn; DESIGN.md
4.26): brute force over every (query, reference) pair, the fp32 fused arithmetic reproduced exactly.

    dist2(i, j) = fmaf(dz, dz, fmaf(dx, dx, dy * dy)),  d = refs[j] - queries[i]  in fp32

The differences and dy * dy are single fp32 operations (the float64 product of two fp32 values is exact, so rounding it to fp32
is the fp32 product).  A fused multiply-add rounds the EXACT a * a + b once.  In float64 a * a is exact but the sum is rounded,
and rounding that to fp32 again can land on the wrong side of an fp32 midpoint; so the float64 sum is made a round-to-ODD one
with its TwoSum error term (an inexact sum whose last bit is even moves one step towards the error), after which the second
rounding is the rounding of the exact value: float64 carries more than two bits beyond fp32.

Rows are ordered by (dist2, id): one 64-bit key per pair, the distance's bits (non-negative floats order like their bits) above
the id.  Masks are applied by index-selecting the arrays and mapping the ids back.
"""
import numpy as np

EMPTY = np.uint64(0x7F800000FFFFFFFF)  # (+inf, id 0xFFFFFFFF): what pads a row, above every pair with a finite distance


def _fma_sq(a, b):
    """fp32 fmaf(a, a, b) for fp32 arrays a and b >= 0, exactly"""
    p = a.astype(np.float64) * a.astype(np.float64)  # exact: 48 bits
    b = b.astype(np.float64)
    s = p + b
    bb = s - p
    err = (p - (s - bb)) + (b - bb)  # TwoSum: p + b == s + err exactly
    bits = s.view(np.int64)
    even = (bits & 1) == 0
    bits = bits + np.where(even & (err > 0), 1, 0) - np.where(even & (err < 0), 1, 0)  # (s > 0 wherever err != 0)
    return bits.view(np.float64).astype(np.float32)


def dist2_matrix(queries, refs):
    """float32 [Pq, Pr] of the definition above"""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    r = np.asarray(refs, np.float32).reshape(-1, 3)
    dx = r[None, :, 0] - q[:, None, 0]
    dy = r[None, :, 1] - q[:, None, 1]
    dz = r[None, :, 2] - q[:, None, 2]
    yy = (dy.astype(np.float64) * dy.astype(np.float64)).astype(np.float32)
    return _fma_sq(dz, _fma_sq(dx, yy))


def knn_rows(queries, refs, k, query_keep=None, ref_keep=None, exclude_self=False, chunk=512):
    """(idx int32 [Pq,k], dist2 float32 [Pq,k]): per query the k smallest (dist2, id) pairs over the kept references, ascending;
    -1 / +inf where there is none, and for a query that is not kept.  exclude_self: reference i is left out of row i."""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    r = np.asarray(refs, np.float32).reshape(-1, 3)
    Pq, Pr = len(q), len(r)
    if exclude_self:
        assert Pq == Pr and np.array_equal(q, r)
    qid = np.arange(Pq) if query_keep is None else np.flatnonzero(np.asarray(query_keep))
    rid = np.arange(Pr) if ref_keep is None else np.flatnonzero(np.asarray(ref_keep))
    keys = np.full((Pq, k), EMPTY, np.uint64)
    rsel = r[rid]
    for a in range(0, len(qid), chunk):
        rows = qid[a:a + chunk]
        d = dist2_matrix(q[rows], rsel)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rid.astype(np.uint64)[None, :]
        if exclude_self:
            key[rows[:, None] == rid[None, :]] = EMPTY
        key = np.concatenate([key, np.full((len(rows), k), EMPTY, np.uint64)], 1)
        keys[rows] = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    dist2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx.reshape(Pq, k), dist2.reshape(Pq, k)


def majority_labels(idx, labels, dist2=None, max_dist2=None):
    """(label int64 [Pq], count int32 [Pq]): per row the label most entries carry, the lowest among equals; an entry counts
    with idx >= 0, labels[idx] >= 0 and dist2 <= max_dist2.  -1 / 0 for a row without one."""
    idx = np.asarray(idx)
    labels = np.asarray(labels, np.int64)
    out = np.full(len(idx), -1, np.int64)
    cnt = np.zeros(len(idx), np.int32)
    for i, row in enumerate(idx):
        ok = row >= 0
        if max_dist2 is not None:
            ok &= np.asarray(dist2)[i] <= np.float32(max_dist2)
        got = labels[row[ok]] if len(labels) else np.zeros(0, np.int64)
        got = got[got >= 0]
        if len(got):
            vals, n = np.unique(got, return_counts=True)  # ascending values: argmax takes the lowest of equals
            out[i], cnt[i] = vals[np.argmax(n)], n.max()
    return out, cnt


def complete_labels(xyz, labels, k=8, max_dist2=None, selection=None):
    labels = np.asarray(labels, np.int64)
    sel = np.ones(len(labels), bool) if selection is None else np.asarray(selection, bool)
    have, ask = (labels >= 0) & sel, (labels < 0) & sel
    idx, dist2 = knn_rows(xyz, xyz, k, query_keep=ask, ref_keep=have)
    found, _ = majority_labels(idx, labels, dist2, max_dist2)
    return np.where(labels >= 0, labels, found)


def mean_distance(dist2):
    dist2 = np.asarray(dist2, np.float32)
    finite = np.isfinite(dist2)
    n = finite.sum(1)
    total = np.where(finite, np.sqrt(dist2, where=finite, out=np.zeros_like(dist2)), np.float32(0)).sum(1, dtype=np.float32)
    return np.where(n > 0, total / np.maximum(n, 1).astype(np.float32), np.float32(np.inf)).astype(np.float32)


def statistical_outliers(points, k=16, ratio=2.0, selection=None):
    _, dist2 = knn_rows(points, points, k, query_keep=selection, ref_keep=selection, exclude_self=True)
    score = mean_distance(dist2).astype(np.float64)
    finite = np.isfinite(score)
    n = finite.sum()
    mu = score[finite].sum() / max(n, 1)
    sigma = np.sqrt(((score[finite] - mu) ** 2).sum() / max(n - 1, 1))
    return finite & (score > mu + ratio * sigma)
