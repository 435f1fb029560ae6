"""A numpy restatement of the two entries of csrc/segment.hip (include/goi_raster.h: goi_knn_segment_edges,
goi_knn_segment_components), written out as the definitions, slowly and plainly.

The gate is in float32 with exact fused arithmetic: d = 0, then d = fmaf(e_c, e_c, d) for c = 0 .. S-1 with e_c = f[i,c] - f[j,c]
(`_fma_sq` of tests/knn_graph_reference.py is exactly that step).  The partition is a sequential union-find over the undirected
graph of the joining edges."""
from __future__ import annotations

import numpy as np

from tests.knn_graph_reference import _fma_sq


def valid_edges(idx):
    """bool [P,k]: 0 <= idx[i,m] < P and idx[i,m] != i"""
    idx = np.asarray(idx, np.int32)
    P = idx.shape[0]
    return (idx >= 0) & (idx < P) & (idx != np.arange(P, dtype=np.int64)[:, None])


def feature_dist2(f, idx, dtype=np.float32):
    """[P,k]: d of the module docstring per entry (0 for an entry that is no valid edge).  float32: the kernel's chain with
    exact fmaf; float64: the plain sum of squares of the float32 differences' float64 values."""
    f = np.asarray(f, np.float32)
    P, S = f.shape
    ok = valid_edges(idx)
    j = np.where(ok, idx, 0).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype == np.float64:
            e = f.astype(np.float64)[:, None, :] - f.astype(np.float64)[j]
            d = np.zeros(j.shape, np.float64)
            for c in range(S):
                d = d + e[:, :, c] * e[:, :, c]
            return np.where(ok, d, 0.0)
        d = np.zeros(j.shape, np.float32)
        for c in range(S):
            e = f[:, None, c] - f[j, c]  # float32 - float32: rounded once
            nan = np.isnan(e) | np.isnan(d)
            step = _fma_sq(np.where(nan, np.float32(0), e), np.where(nan, np.float32(0), d))  # (_fma_sq's TwoSum takes no NaN)
            d = np.where(nan, np.float32(np.nan), step)
        return np.where(ok, d, np.float32(0))


def edges(idx, features=None, tau=np.inf, dist2=None, max_dist2=None, labels=None, rows=None, mutual=False):
    """uint8 [P,k]: the definition of goi_knn_segment_edges, clause by clause"""
    idx = np.asarray(idx, np.int32)
    P, k = idx.shape
    assert not np.isnan(tau) and (max_dist2 is None or dist2 is not None)
    ok = valid_edges(idx)
    j = np.where(ok, idx, 0).astype(np.int64)
    if rows is not None:
        rows = np.asarray(rows) != 0
        ok &= rows[:, None] & rows[j]
    if labels is not None:
        labels = np.asarray(labels, np.int64)
        ok &= (labels[:, None] >= 0) & (labels[:, None] == labels[j])
    if max_dist2 is not None:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(dist2, np.float32) <= np.float32(max_dist2)
    if features is not None:
        with np.errstate(invalid="ignore"):
            ok &= feature_dist2(features, idx) <= np.float32(tau)  # a NaN never passes `<=`
    if mutual:
        back = (idx[j] == np.arange(P, dtype=np.int64)[:, None, None]).any(axis=2)  # i is in row j's list
        ok &= back
    return ok.astype(np.uint8)


def components(idx, join=None, rows=None, min_size=1):
    """(root, size, label int32 [P], count): a plain sequential union-find, then the outputs as goi_knn_segment_components
    defines them"""
    idx = np.asarray(idx, np.int32)
    P, k = idx.shape
    assert min_size >= 1
    kept = np.ones(P, bool) if rows is None else np.asarray(rows) != 0
    ok = valid_edges(idx)
    if join is not None:
        ok &= np.asarray(join) != 0
    parent = list(range(P))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, m in zip(*np.nonzero(ok)):
        j = int(idx[i, m])
        if not (kept[i] and kept[j]):
            continue
        a, b = find(int(i)), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)  # the smaller id stays the root: the root of a finished tree is its minimum
    root = np.array([find(i) if kept[i] else -1 for i in range(P)], np.int32).reshape(P)
    size = np.zeros(P, np.int32)
    members = np.bincount(root[root >= 0], minlength=P) if P else np.zeros(0, np.int64)
    size[root >= 0] = members[root[root >= 0]]
    keep_root = (root == np.arange(P)) & (size >= min_size)
    rank = np.cumsum(keep_root) - keep_root  # exclusive: the dense rank in ascending root
    label = np.full(P, -1, np.int32)
    in_kept = (root >= 0) & (size >= min_size)
    label[in_kept] = rank[root[in_kept]]
    return root, size, label, int(keep_root.sum())


def partition(root):
    """the partition as a set of frozensets of row ids (rows with root -1 are in none)"""
    groups = {}
    for i, r in enumerate(np.asarray(root).tolist()):
        if r >= 0:
            groups.setdefault(r, []).append(i)
    return {frozenset(g) for g in groups.values()}
