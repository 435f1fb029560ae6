"""Test-only numpy restatement of sklearn.cluster.DBSCAN(eps, min_samples).fit(X) with the neighbour test of
csrc/dbscan.hip: d2 = fma(dz, dz, fma(dy, dy, dx * dx)) <= eps32 * eps32 in fp32, dx = xi - xj (y, z alike).

dbscan_reference shares nothing with the kernel's grid: a float64 k-d tree (scipy) proposes candidate pairs within
eps (1 + 2^-18), which contains every fp32 neighbour, and every decision is then taken by the fp32 form above.  Counts of
points whose float64 counts at eps (1 -+ 2^-18) agree are exact without the form.  Clusters are the connected components of
the core-core neighbour graph, merged chunk by chunk; numbering by smallest core index; a border point takes the smallest
label among its core neighbours; the rest is -1.

dbscan_brute is a second, independent statement of the same definition from the dense neighbour matrix (no tree, no
chunked merging), for n <= 10 000; it also takes the alternative forms of d2_alt, which the tests of the adversarial cases
(tests/dbscan_cases.py) use to show that an input tells the kernel's form from its near misses.

fma is exact for every fp32 input (_fma32: exact float64 product, TwoSum with the addend, round to odd, round to fp32), so
the restatement is the kernel's arithmetic for arbitrary floats, on or off a lattice.  Off the lattice the oracle is this
fp32 form and not sklearn, whose float64 distances decide threshold pairs differently.
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
    """fl32(a * b + c) of fp32 arrays with ONE rounding, as the hardware fma.  a * b is exact in float64 (48 bits); TwoSum
    gives the float64 sum s and its exact error e; when e != 0 and s is even, s moves one step towards e (round to odd), so
    the 53-bit value keeps on which side of any fp32 midpoint the exact sum lies; the cast then rounds it once."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
    c = np.asarray(c, F32).astype(F64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _fma32_double_rounding(a, b, c):
    """The emulation this module used before: one rounding of the float64 value, i.e. two roundings.  Kept for the test
    that shows where it differs from _fma32."""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def d2_form(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp32 d2 of the rows of a and b ([..., 3] float32) in the kernel's form."""
    a, b = a.astype(F32, copy=False), b.astype(F32, copy=False)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return _fma32(dz, dz, _fma32(dy, dy, dx * dx))


ALT_KINDS = ("plain", "reversed", "float64")


def d2_alt(a: np.ndarray, b: np.ndarray, kind: str) -> np.ndarray:
    """d2 of the rows of a and b in a form the kernel does NOT use: 'plain' (dx*dx + dy*dy) + dz*dz with every operation
    rounded to fp32; 'reversed' fma(dx, dx, fma(dy, dy, dz * dz)); 'float64' the sum of squares of the float64 differences
    (float64 result: what a float64 library computes).  Only the tests of the cases use it, never an assertion about the
    device."""
    a, b = a.astype(F32, copy=False), b.astype(F32, copy=False)
    if kind == "float64":
        d = a.astype(F64) - b.astype(F64)
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    if kind == "plain":
        return (dx * dx + dy * dy) + dz * dz
    if kind == "reversed":
        return _fma32(dx, dx, _fma32(dy, dy, dz * dz))
    raise ValueError(f"d2_alt: unknown kind {kind!r}")


def is_neighbour(a: np.ndarray, b: np.ndarray, eps: float, kind: str = "kernel") -> np.ndarray:
    """The neighbour decision of the rows of a and b: the kernel's (kind 'kernel': d2_form <= fl32(eps32 * eps32)) or an
    alternative form's (the fp32 kinds against the same fp32 threshold, 'float64' against the exact square of eps32)."""
    eps32 = F32(eps)
    if kind == "kernel":
        return d2_form(a, b) <= F32(eps32 * eps32)
    if kind == "float64":
        return d2_alt(a, b, kind) <= F64(eps32) * F64(eps32)
    return d2_alt(a, b, kind) <= F32(eps32 * eps32)


BRUTE_ROWS = 256
BRUTE_MAX_N = 10_000


def brute_neighbours(X, eps: float, kind: str = "kernel"):
    """The whole neighbour relation as a boolean CSR matrix [n, n], from dense row blocks of BRUTE_ROWS rows.  A float64
    sum of squares settles every pair further than 2^-16 (relative) from eps^2, about 2^8 times the fp32 forms' rounding;
    the pairs inside that band are decided by is_neighbour(kind)."""
    X = np.ascontiguousarray(X, dtype=F32)
    n = X.shape[0]
    assert n <= BRUTE_MAX_N, "brute_neighbours is quadratic: n <= 10 000"
    e2 = F64(F32(eps)) * F64(F32(eps))
    Xd = X.astype(F64)
    rows, cols = [], []
    for s in range(0, n, BRUTE_ROWS):
        d = Xd[s:s + BRUTE_ROWS, None, :] - Xd[None, :, :]
        q = np.einsum("ijk,ijk->ij", d, d)
        near = q <= e2 * (1 - 2.0 ** -16)
        i, j = np.nonzero((q <= e2 * (1 + 2.0 ** -16)) & ~near)
        near[i, j] = is_neighbour(X[s + i], X[j], eps, kind)
        i, j = np.nonzero(near)
        rows.append(i + s)
        cols.append(j)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return coo_matrix((np.ones(len(rows), bool), (rows, cols)), shape=(n, n)).tocsr()


def labels_from_neighbours(nb, min_samples: int):
    """(labels int64 [n], core bool [n]) from a symmetric boolean neighbour matrix with a true diagonal: core = row count
    >= min_samples; clusters = components of the core-core graph numbered by smallest core index; a border point takes
    the smallest label among its core neighbours."""
    n = nb.shape[0]
    core = np.asarray(nb.sum(axis=1)).reshape(-1) >= min_samples
    labels = np.full(n, -1, np.int64)
    cidx = np.nonzero(core)[0]
    if len(cidx) == 0:
        return labels, core
    _, comp = connected_components(nb[cidx][:, cidx], directed=False)
    _, first = np.unique(comp, return_index=True)  # first (smallest) core position of every component
    number = np.empty(len(first), np.int64)
    number[np.argsort(first)] = np.arange(len(first))
    labels[cidx] = number[comp]
    to_core = nb[:, cidx].tocsr()
    for b in np.nonzero(~core)[0]:
        hit = to_core.indices[to_core.indptr[b]:to_core.indptr[b + 1]]
        if len(hit):
            labels[b] = labels[cidx[hit]].min()
    return labels, core


def dbscan_brute(X, eps: float, min_samples: int, kind: str = "kernel"):
    """(labels, core) of DBSCAN from the dense neighbour matrix, for n <= 10 000; kind selects the kernel's form or one of
    ALT_KINDS (the mutation checks)."""
    X = np.ascontiguousarray(X, dtype=F32)
    if X.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    return labels_from_neighbours(brute_neighbours(X, eps, kind), min_samples)


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
