"""numpy restatements of goi_hyperplane_amd.mesh (csrc/mesh.hip) and the meshes its tests run on.

The restatements use exactly the arithmetic the module documents: float32 operations rounded once each, float64 sums in a
fixed order.  Sequential sums are written as rank-by-rank loops: pass r adds every run's r-th member, so each run is summed
in its own order while numpy still works on whole arrays.  Nothing here imports the package under test.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import field_reference as fr

F32 = np.float32


# ---- components ---------------------------------------------------------------------------------------------------------------
def components(faces, n_vertices, alive=None):
    """-> (vertex_label int32 [V], face_label int32 [F]): the smallest vertex index of the component, -1 for an unnamed vertex;
    the label of a face is that of its first vertex.  Min-label propagation with pointer jumping until nothing changes."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = int(n_vertices)
    g = f if alive is None else f[np.asarray(alive, dtype=bool)]
    label = np.arange(V, dtype=np.int64)
    while True:
        m = label[g].min(axis=1) if len(g) else np.zeros(0, np.int64)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, g[:, k], m)
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    named = np.zeros(V, dtype=bool)
    named[g.reshape(-1)] = True
    vlabel = np.where(named, label, -1).astype(np.int32)
    flabel = vlabel[f[:, 0]] if len(f) else np.zeros(0, np.int32)
    return vlabel, flabel.astype(np.int32)


# ---- clean --------------------------------------------------------------------------------------------------------------------
def cross_f32(v, f):
    """(v1 - v0) x (v2 - v0) per face in float32, every operation rounded once."""
    v = np.asarray(v, dtype=F32)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        u, w = b - a, c - a
        return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                         u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)


def null_faces(v, f):
    rep = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    bad = ~np.isfinite(np.asarray(v, dtype=F32)).all(axis=1)
    n = cross_f32(v, f)
    return rep | bad[f].any(axis=1) | ((n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] == 0))


def first_of_each_set(tri, alive):
    """alive and no lower alive row holds the same set of three indices."""
    out = np.zeros(len(tri), dtype=bool)
    idx = np.nonzero(alive)[0]
    if idx.size:
        _, first = np.unique(np.sort(tri[idx], axis=1), axis=0, return_index=True)  # return_index: the first occurrence
        out[idx[first]] = True
    return out


def box_d2(lo, hi):
    """float64 sum, x y z, of the squares of the float32 extents."""
    e = (np.asarray(hi, dtype=F32) - np.asarray(lo, dtype=F32)).astype(np.float64)
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def clean(vertices, faces, colors=None, min_faces=64, min_diag=0.2, info=None):
    """-> (vertices, faces, colors, vertex_index, face_index).  info (a dict) receives the per-component figures."""
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    alive = ~null_faces(v, f) if len(f) else np.zeros(0, bool)
    alive = first_of_each_set(f, alive)
    vlabel, flabel = components(f, V, alive)
    keep = np.zeros(len(f), dtype=bool)
    named = vlabel >= 0
    if named.any():
        roots = np.unique(vlabel[named])
        nfaces = np.bincount(flabel[alive], minlength=V)[roots]
        lo = np.full((V, 3), np.inf, F32)
        hi = np.full((V, 3), -np.inf, F32)
        np.minimum.at(lo, vlabel[named], v[named])
        np.maximum.at(hi, vlabel[named], v[named])
        d2c = box_d2(lo[roots], hi[roots])
        d2m = box_d2(v[named].min(axis=0), v[named].max(axis=0))
        ckeep = (nfaces >= int(min_faces)) & ~(d2c < float(min_diag) * float(min_diag) * d2m)
        if info is not None:
            info.update(roots=roots, faces=nfaces, diag=np.sqrt(d2c / d2m) if d2m > 0 else np.zeros(len(roots)), keep=ckeep,
                        nulls_and_duplicates=int(len(f) - alive.sum()))
        good = np.zeros(V, dtype=bool)
        good[roots[ckeep]] = True
        keep = alive.copy()
        keep[alive] = good[flabel[alive]]
    used = np.zeros(V, dtype=bool)
    used[f[keep].reshape(-1)] = True
    new = np.cumsum(used) - 1
    vidx, fidx = np.nonzero(used)[0].astype(np.int32), np.nonzero(keep)[0].astype(np.int32)
    col = None if colors is None else np.asarray(colors, dtype=F32).reshape(-1, 3)[vidx]
    return v[vidx], new[f[keep]].astype(np.int32).reshape(-1, 3), col, vidx, fidx


# ---- decimate -----------------------------------------------------------------------------------------------------------------
def members(vertices, faces):
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    named = np.zeros(len(v), dtype=bool)
    named[np.asarray(faces, dtype=np.int64).reshape(-1)] = True
    return named & np.isfinite(v).all(axis=1)


def cell_keys(vertices, member, n):
    """int64 [V]: the key of every member's cell at n divisions (others: -1); plus (lo, cell) for the box checks."""
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    key = np.full(len(v), -1, dtype=np.int64)
    if not member.any():
        return key, np.zeros(3, F32), F32(0)
    m = v[member]
    lo = m.min(axis=0)
    e = F32((m.max(axis=0) - lo).max())
    cell = F32(e / F32(n))
    if not e > 0:
        key[member] = 0
        return key, lo, cell
    with np.errstate(all="ignore"):
        q = np.minimum(np.floor(((m - lo) / cell).astype(F32)), F32(n - 1)).astype(np.int64)
    key[member] = (q[:, 0] * n + q[:, 1]) * n + q[:, 2]
    return key, lo, cell


def distinct_cells(key, f):
    k = key[f]
    return (k >= 0).all(axis=1) & (k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])


def probe_count(vertices, faces, n):
    """count(n): faces whose three vertices are members in three distinct cells, before the dedup."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    key, _, _ = cell_keys(vertices, members(vertices, f), n)
    return int(distinct_cells(key, f).sum())


def run_means(values, order, starts, counts):
    """float64 sum of every run's rows in the run's order (rank by rank), / count, rounded to float32."""
    acc = np.zeros((len(starts), values.shape[1]), dtype=np.float64)
    for r in range(int(counts.max()) if len(counts) else 0):
        has = counts > r
        acc[has] += values[order[starts[has] + r]].astype(np.float64)
    return (acc / counts[:, None].astype(np.float64)).astype(F32)


def bisect_divisions(count, target, hi=1024):
    if count(hi) <= target:
        return hi
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count(mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo


def decimate(vertices, faces, colors=None, divisions=None, target_faces=None, info=None):
    """-> (vertices, faces, colors, divisions, cluster)."""
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    c = None if colors is None else np.asarray(colors, dtype=F32).reshape(-1, 3)
    assert (divisions is None) != (target_faces is None)
    if divisions is None:
        if len(f) <= target_faces:
            return v, f.astype(np.int32), c, 0, np.arange(len(v), dtype=np.int32)
        divisions = bisect_divisions(lambda n: probe_count(v, f, n), target_faces)
    n = int(divisions)
    member = members(v, f)
    key, lo, cell = cell_keys(v, member, n)
    order = np.argsort(np.where(member, key, np.int64(n) ** 3), kind="stable")[:int(member.sum())]  # (key, vertex)
    skey = key[order]
    head = np.ones(len(order), dtype=bool)
    head[1:] = skey[1:] != skey[:-1]
    starts = np.nonzero(head)[0]
    counts = np.diff(np.append(starts, len(order)))
    vcell = np.full(len(v), -1, dtype=np.int64)
    vcell[order] = np.cumsum(head) - 1
    alive = distinct_cells(key, f)
    tri = np.where(alive[:, None], vcell[f], 0)
    n_distinct = int(alive.sum())
    alive = first_of_each_set(tri, alive)
    used = np.zeros(len(starts), dtype=bool)
    used[tri[alive].reshape(-1)] = True
    new = np.cumsum(used) - 1
    out_v = run_means(v, order, starts, counts)[used]
    out_c = None if c is None else run_means(c, order, starts, counts)[used]
    cluster = np.where((vcell >= 0) & used[np.maximum(vcell, 0)], new[np.maximum(vcell, 0)], -1).astype(np.int32)
    if info is not None:
        info.update(cells=len(starts), distinct=n_distinct, lo=lo, cell=cell, keys=skey[starts][used], n=n)
    return out_v, new[tri[alive]].astype(np.int32).reshape(-1, 3), out_c, n, cluster


# ---- normals ------------------------------------------------------------------------------------------------------------------
def _normalise(s, dtype):
    eps = dtype(1e-20)
    with np.errstate(all="ignore"):
        dot = ((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]).astype(dtype)
        ok = dot > eps
        s = np.where(ok[:, None], s, np.array([0, 0, 1], dtype=dtype))
        dot = np.where(ok, dot, dtype(1))
        return (s / np.sqrt(np.maximum(dot, eps))[:, None]).astype(dtype)


def vertex_normals(vertices, faces, dtype=F32, order="face"):
    """Sum of the incident faces' cross products per vertex, then auto_normal's normalisation.  order: "face" sums a vertex's
    corners in ascending (face, corner) order (the device's); "corner" in ascending (corner, face) order (the reference's three
    scatter_adds on the CPU).  dtype float64: the truth both are measured against (cross products from the float32 inputs)."""
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3).astype(dtype)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        u, w = b - a, c - a
        fn = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                       u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1).astype(dtype)
    if order == "face":
        vert, face = f.reshape(-1), np.repeat(np.arange(len(f)), 3)
    else:
        vert, face = f.T.reshape(-1), np.tile(np.arange(len(f)), 3)
    srt = np.argsort(vert, kind="stable")
    vert, face = vert[srt], face[srt]
    counts = np.bincount(vert, minlength=len(v))
    starts = np.cumsum(counts) - counts
    s = np.zeros((len(v), 3), dtype=dtype)
    with np.errstate(all="ignore"):
        for r in range(int(counts.max()) if len(f) else 0):
            has = counts > r
            s[has] = (s[has] + fn[face[starts[has] + r]]).astype(dtype)
    return _normalise(s, dtype)


def cancellation(vertices, faces):
    """float64 |sum| / sum |contribution| per vertex (1 where nothing is summed): small where the faces cancel."""
    v = np.asarray(vertices, dtype=F32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    s, mag = np.zeros((len(v), 3)), np.zeros(len(v))
    for k in range(3):
        np.add.at(s, f[:, k], fn)
        np.add.at(mag, f[:, k], np.linalg.norm(fn, axis=1))
    return np.where(mag > 0, np.linalg.norm(s, axis=1) / np.where(mag > 0, mag, 1), 1.0)


# ---- meshes -------------------------------------------------------------------------------------------------------------------
def blobs_grid(shape=(40, 36, 32), n=48, seed=5):
    """The maximum of n balls 2 - |p - c| / r: centres uniform in [2, shape - 3], radii log-uniform in 0.9 .. 6.0."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(2.0, np.array(shape, dtype=np.float64) - 3.0, size=(n, 3))
    radii = np.exp(rng.uniform(np.log(0.9), np.log(6.0), size=n))
    p = fr._points(shape)
    g = np.full(shape, -np.inf)
    for c, r in zip(centres, radii):
        g = np.maximum(g, 2.0 - np.linalg.norm(p - c, axis=-1) / r)
    return g.astype(F32), 1.0


@functools.lru_cache(maxsize=None)
def _grid_mesh(name):
    grid, thresh = {"sphere": fr.sphere_grid, "torus": fr.torus_grid, "two_spheres": fr.two_spheres_grid, "equal": fr.equal_grid,
                    "blobs": blobs_grid, "noisy24": lambda: fr.noisy_grid((24, 24, 24)),
                    "sphere48": lambda: fr.sphere_grid((48, 48, 48), (23.3, 23.6, 23.1), 19.2)}[name]()
    v, f, c = fr.marching_tets(grid, thresh, fr.grid_attributes(grid.shape))
    for a in (v, f, c):
        a.setflags(write=False)
    return v, f, c


def grid_mesh(name):
    """(vertices float32, faces int32, colors float32) of the named analytic grid's iso-surface; computed once, read-only."""
    return _grid_mesh(name)


def strip(n_triangles, lo, hi, seed=None):
    """A zig-zag strip of n triangles from corner lo to corner hi of a box (n + 2 vertices; one component).  seed: the vertex
    numbering is a random permutation, which makes the union chains long."""
    k = np.arange(n_triangles + 2)
    t = (k / (n_triangles + 1))[:, None]
    v = np.asarray(lo, dtype=np.float64) + t * (np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))
    v[:, 1] += np.where(k % 2 == 0, 0.37, -0.41)  # off the diagonal: no zero areas
    i = np.arange(n_triangles)
    f = np.stack([i, i + 1, i + 2], axis=1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    v = v.astype(F32)
    if seed is not None:
        perm = np.random.default_rng(seed).permutation(len(v))
        w = np.empty_like(v)
        w[perm] = v
        v, f = w, perm[f]
    return v, f.astype(np.int32)


def concat(*meshes):
    """Meshes (vertices, faces[, colors]) side by side; colours where all have them."""
    vs, fs, cs, base = [], [], [], 0
    for m in meshes:
        vs.append(np.asarray(m[0], dtype=F32))
        fs.append(np.asarray(m[1], dtype=np.int64) + base)
        cs.append(m[2] if len(m) > 2 else None)
        base += len(m[0])
    col = None if any(c is None for c in cs) else np.concatenate(cs).astype(F32)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32), col


@functools.lru_cache(maxsize=None)
def dirty_blobs():
    """blobs + a 20-triangle strip across its box (removed by the face count alone) + dirt: a face with a repeated index, two
    more copies of face 7 in another rotation and in the other orientation, and an unreferenced NaN vertex."""
    v, f, c = grid_mesh("blobs")
    sv, sf = strip(20, v.min(axis=0), v.max(axis=0))
    sc = np.linspace(0.0, 1.4, sv.size, dtype=F32).reshape(-1, 3)
    v, f, c = concat((v, f, c), (sv, sf, sc))
    dirt = np.array([[f[3, 0], f[3, 1], f[3, 0]], [f[7, 1], f[7, 2], f[7, 0]], [f[7, 0], f[7, 2], f[7, 1]]], dtype=np.int32)
    f = np.concatenate([f[:100], dirt[:2], f[100:], dirt[2:]])
    v = np.concatenate([v, np.array([[np.nan, 0, 0]], dtype=F32)])
    c = np.concatenate([c, np.zeros((1, 3), F32)])
    for a in (v, f, c):
        a.setflags(write=False)
    return v, f, c


@functools.lru_cache(maxsize=None)
def permuted_strip():
    return strip(4096, (0, 0, 0), (50, 3, 7), seed=11)
