"""Test-only numpy restatement of sklearn.cluster.DBSCAN(eps, min_samples).fit(X) with the neighbour test of
csrc/dbscan.hip: d2 = fma(dz, dz, fma(dy, dy, dx * dx)) <= eps32 * eps32 in fp32, dx = xi - xj (y, z alike).

It shares nothing with the kernel's grid: a float64 k-d tree (scipy) proposes candidate pairs within eps (1 + 2^-18), which
contains every fp32 neighbour, and every decision is then taken by the fp32 form above.  Counts of points whose float64
counts at eps (1 -+ 2^-18) agree are exact without the form.  Clusters are the connected components of the core-core
neighbour graph, merged chunk by chunk; numbering by smallest core index; a border point takes the smallest label among its
core neighbours; the rest is -1.

fma is emulated as one rounding of the float64 value a*b + c: a*b of two fp32 numbers is exact in float64, and the sum is
exact whenever it fits 53 bits (always for points on a 2^-10 lattice within |x| < 2^10, which is what the tests use);
otherwise the double rounding could differ from a true fma in rare ties.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

F32, F64 = np.float32, np.float64
REL = 2.0 ** -18
CHUNK_PAIRS = 4_000_000


def _fma32(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def d2_form(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp32 d2 of the rows of a and b ([..., 3] float32) in the kernel's form."""
    a, b = a.astype(F32, copy=False), b.astype(F32, copy=False)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return _fma32(dz, dz, _fma32(dy, dy, dx * dx))


def _pairs(tree_a: cKDTree, tree_b: cKDTree, r: float):
    """All (i in a, j in b) with float64 distance <= r, as two int64 arrays."""
    m = tree_a.sparse_distance_matrix(tree_b, r, output_type="ndarray")
    return m["i"].astype(np.int64), m["j"].astype(np.int64)


def _chunks(idx: np.ndarray, per_point: float):
    step = max(1, int(CHUNK_PAIRS / max(per_point, 1.0)))
    for s in range(0, len(idx), step):
        yield idx[s:s + step]


def dbscan_reference(X, eps: float, min_samples: int):
    """(labels int64 [n], core bool [n]) for float32 X [n, 3]."""
    X = np.ascontiguousarray(X, dtype=F32)
    n = X.shape[0]
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    eps32 = F32(eps)
    eps2 = F32(eps32 * eps32)
    Xd = X.astype(F64)
    r_lo, r_hi = float(eps32) * (1 - REL), float(eps32) * (1 + REL)
    tree = cKDTree(Xd)
    c_lo = tree.query_ball_point(Xd, r_lo, return_length=True, workers=-1)
    c_hi = tree.query_ball_point(Xd, r_hi, return_length=True, workers=-1)
    core = c_lo >= min_samples
    amb = np.nonzero((c_lo < min_samples) & (c_hi >= min_samples))[0]
    for part in _chunks(amb, float(c_hi[amb].mean()) if len(amb) else 1.0):
        i, j = _pairs(cKDTree(Xd[part]), tree, r_hi)
        ok = d2_form(X[part[i]], X[j]) <= eps2
        core[part] |= np.bincount(i[ok], minlength=len(part)) >= min_samples

    labels = np.full(n, -1, np.int64)
    cidx = np.nonzero(core)[0]
    if len(cidx):
        ctree = cKDTree(Xd[cidx])
        comp = np.arange(len(cidx))
        for part in _chunks(np.arange(len(cidx)), float(c_hi[cidx].mean())):
            i, j = _pairs(cKDTree(Xd[cidx[part]]), ctree, r_hi)
            ok = d2_form(X[cidx[part[i]]], X[cidx[j]]) <= eps2
            a, b = comp[part[i[ok]]], comp[j[ok]]
            sel = a != b
            if sel.any():
                g = coo_matrix((np.ones(int(sel.sum()), np.int8), (a[sel], b[sel])), shape=(len(cidx), len(cidx)))
                _, merged = connected_components(g, directed=False)
                comp = merged[comp]
        # number the components by their smallest core index (cidx is ascending)
        first = np.full(comp.max() + 1, len(cidx), np.int64)
        np.minimum.at(first, comp, np.arange(len(cidx)))
        order = np.argsort(first[first < len(cidx)], kind="stable")
        used = np.nonzero(first < len(cidx))[0]
        number = np.empty(comp.max() + 1, np.int64)
        number[used[order]] = np.arange(len(used))
        labels[cidx] = number[comp]
        # border points: smallest label among core neighbours
        bidx = np.nonzero(~core)[0]
        if len(bidx):
            for part in _chunks(bidx, float(c_hi[bidx].mean())):
                i, j = _pairs(cKDTree(Xd[part]), ctree, r_hi)
                ok = d2_form(X[part[i]], X[cidx[j]]) <= eps2
                best = np.full(len(part), np.iinfo(np.int64).max, np.int64)
                np.minimum.at(best, i[ok], labels[cidx[j[ok]]])
                labels[part] = np.where(best == np.iinfo(np.int64).max, -1, best)
    return labels, core


def lattice_blobs(rng, n: int, centers: int = 4, noise: float = 0.1, spread: float = 0.6, extent: float = 8.0,
                  unit: float = 2.0 ** -10):
    """Clustered points with uniform noise, rounded to a 2^-10 lattice (float32 [n, 3]); the test data of the restatement."""
    n_noise = int(n * noise)
    c = rng.uniform(-extent, extent, size=(centers, 3))
    which = rng.integers(0, centers, size=n - n_noise)
    pts = np.concatenate([c[which] + rng.normal(0.0, spread, size=(n - n_noise, 3)),
                          rng.uniform(-extent - 2, extent + 2, size=(n_noise, 3))])
    pts = pts[rng.permutation(n)]
    return (np.round(pts / unit) * unit).astype(F32)
