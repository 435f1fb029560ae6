"""Named adversarial inputs for exact DBSCAN (csrc/dbscan.hip): point sets whose neighbour decisions sit ON the threshold
d2 <= eps32 * eps32 of the kernel's fp32 form, off any lattice, far from the origin, at the grid's edges and along chains.

Every case is a function of a seed that returns a Case: a tuple (points float32 [n, 3], eps, min_samples), n <= 30 000,
with the construction's bookkeeping in .meta (used by tests/test_dbscan_cases_cpu.py to show that the case deserves its
name, never by an assertion about the device).  Points are built as fp32 values where they lie (never built at the origin
and translated) and arrive in a random permutation.

Building blocks
  * a BOND is a pair of points whose d2 in the kernel's form (tests/dbscan_reference.d2_form) is exactly one of
    pred(eps2), eps2, succ(eps2) -- classes -1, 0, +1; eps2 = fl32(eps32 * eps32).  Classes -1 and 0 are neighbours, +1 is
    not.  _partner() finds the second point: the offset is solved axis by axis from the coarsest coordinate to the finest
    (so that a coordinate of 2 * 10^5, whose fp32 step is 0.045 eps, does not spoil the distance), then all nudges of up to
    +-6 ulps per coordinate are tried and, among those that land in the wanted class, the one on which most alternative
    forms (d2_alt) decide differently from the kernel's form is kept.
  * a MOLECULE is a pair (one bond) or a hinge a-b-c (two bonds at b, angle >= 120 degrees, so a-c is beyond 1.7 eps).
    Molecules sit at the sites of a grid of spacing 5 eps with a jitter of +-0.25 eps and reach at most eps from their
    site, so two molecules stay more than 2 eps apart and the clustering follows from the bond classes alone.
  * bond directions cycle through random, axis (|d| ~ eps ~ 1.73 cells along one axis with 1-4 % across: the partner is
    two cells away, the case for the +-2 window) and the space diagonal.
Class codes in meta["bond_class"]: -1, 0, +1 as above; -2 a plain neighbour (well inside), +2 plainly apart.
"""
from __future__ import annotations

import functools

import numpy as np

from tests.dbscan_reference import ALT_KINDS, d2_alt, d2_form

F32, F64 = np.float32, np.float64
K_NUDGE = 6
SITE = 5.0     # grid spacing of the sites, in eps
JITTER = 0.25  # site jitter, in eps (each axis, each sign)


class Case(tuple):
    """(points, eps, min_samples) with .meta."""

    def __new__(cls, points, eps, min_samples, meta):
        points.setflags(write=False)
        self = super().__new__(cls, (points, float(eps), int(min_samples)))
        self.meta = meta
        return self


def eps2_of(eps):
    e = F32(eps)
    return F32(e * e)


def class_values(eps):
    """(pred(eps2), eps2, succ(eps2)) as fp32."""
    e2 = eps2_of(eps)
    return np.array([np.nextafter(e2, F32(0)), e2, np.nextafter(e2, F32(np.inf))], F32)


def cell_side(eps) -> float:
    """The grid's cell side as goi_semantic_dbscan (csrc/dbscan.hip) computes it (float64)."""
    return float(F64(F32(eps)) / np.sqrt(F64(3.0)) * (1.0 - 1.0 / 4096.0))


def cell_indices(points, eps):
    """Cell coordinates [n, 3] by the documented formula: floor of the fp64 quotient (x - lo) / h, lo the fp32 minimum."""
    p = np.asarray(points, F32).astype(F64)
    return np.floor((p - p.min(axis=0)) / cell_side(eps)).astype(np.int64)


def _step_ulps(x, k):
    """The fp32 values k representable steps from x (k an integer array, either sign)."""
    i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
    o = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F32)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _directions(rng, kinds):
    """Unit vectors [m, 3] for kinds 0 random, 1 axis (1-4 % across), 2 space diagonal (1 % off), 3 the +y axis,
    4 exactly (1, 1, 1) / sqrt(3)."""
    m = len(kinds)
    u = _unit(rng.normal(size=(m, 3)))
    ax = rng.uniform(0.01, 0.04, (m, 3)) * rng.choice([-1.0, 1.0], (m, 3))
    main = np.where(kinds == 3, 1, rng.integers(0, 3, m))
    ax[np.arange(m), main] = np.where(kinds == 3, 1.0, rng.choice([-1.0, 1.0], m))
    dg = rng.choice([-1.0, 1.0], (m, 3)) + rng.uniform(-0.01, 0.01, (m, 3))
    dg[kinds == 4] = 1.0
    axis = (kinds == 1) | (kinds == 3)
    return np.where(axis[:, None], _unit(ax), np.where((kinds >= 2)[:, None], _unit(dg), u))


def _opposed(rng, u, kinds):
    """For every u a direction at >= 130 degrees from it (axis and diagonal kinds: within a few degrees of -u)."""
    m = len(u)
    w = rng.normal(size=(m, 3))
    w = _unit(w - (w * u).sum(1, keepdims=True) * u)
    phi = np.where(kinds == 0, rng.uniform(0.0, np.radians(50.0), m), rng.uniform(0.01, 0.04, m))
    return _unit(-np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * w)


def _first_guess(a, u, eps):
    """fp32 b with |b - a| ~ eps along u: the offset of the coarsest coordinate is rounded first (towards a), the rest is
    rescaled to what is left of eps^2, and the finest coordinate takes the remainder."""
    e = float(F32(eps))
    ad = a.astype(F64)
    order = np.argsort(-np.abs(ad), axis=1, kind="stable")
    rows = np.arange(len(a))
    b = a.copy()
    left = np.full(len(a), e * e)
    t = e * u
    for rank in range(3):
        ax = order[:, rank]
        rest = np.zeros(len(a))
        for r2 in range(rank, 3):
            rest += t[rows, order[:, r2]] ** 2
        want = t[rows, ax] * np.sqrt(left / np.maximum(rest, 1e-300))
        if rank == 2:
            want = np.where(t[rows, ax] < 0, -1.0, 1.0) * np.sqrt(left)
        v = (ad[rows, ax] + want).astype(F32)
        over = (v.astype(F64) - ad[rows, ax]) ** 2 > left
        if rank < 2:  # keep something for the finer axes: step back towards a
            v = np.where(over, _step_ulps(v, np.where(want > 0, -1, 1)), v)
        b[rows, ax] = v
        left = np.maximum(left - (v.astype(F64) - ad[rows, ax]) ** 2, 0.0)
    return b


_K = np.arange(-K_NUDGE, K_NUDGE + 1)
_NUDGES = np.stack(np.meshgrid(_K, _K, _K, indexing="ij"), -1).reshape(-1, 3)


def _partner(rng, a, u, eps, want):
    """For anchors a [m, 3] (fp32), directions u and wanted classes want [m] in {-1, 0, +1}: partners b [m, 3] and the
    class reached [m] (the wanted one where a nudge reaches it, else another threshold class, else 9: no bond)."""
    vals = class_values(eps)
    e2 = vals[1]
    b0 = _first_guess(a, u, eps)
    out, got = b0.copy(), np.full(len(a), 9, np.int64)
    for s in range(0, len(a), 512):
        aa, bb = a[s:s + 512], b0[s:s + 512]
        cand = np.stack([_step_ulps(bb[:, c:c + 1], _NUDGES[None, :, c]) for c in range(3)], -1)  # [m, N, 3]
        d2 = d2_form(aa[:, None, :], cand)
        cls = np.full(d2.shape, 9, np.int64)
        for c, v in zip((-1, 0, 1), vals):
            cls[d2 == v] = c
        i, j = np.nonzero(cls != 9)
        near = d2[i, j] <= e2
        score = np.zeros(len(i))
        for kind in ALT_KINDS:
            d = d2_alt(aa[i], cand[i, j], kind)
            thr = F64(F32(eps)) ** 2 if kind == "float64" else e2
            score += (d <= thr) != near
        score += 10.0 * (cls[i, j] == want[s:s + 512][i]) + rng.uniform(0, 0.5, len(i))
        best = np.full(len(aa), -1.0)
        np.maximum.at(best, i, score)
        pick = score == best[i]
        out[s + i[pick]] = cand[i[pick], j[pick]]
        got[s + i[pick]] = cls[i[pick], j[pick]]
    return out, got


def _cycle_classes(rng, m):
    return rng.permutation(np.arange(m) % 3 - 1)


def _molecules(rng, anchors, eps, n_pairs, kinds=None):
    """Pairs on the first n_pairs anchors and hinges (anchor in the middle) on the others.  Returns points [n, 3], bonds
    [nb, 2], bond classes, bond kinds (0 random, 1 axis, 2 diagonal) and the molecule of every point; molecules with a
    bond that no nudge brought to a threshold class are left out."""
    m = len(anchors)
    kinds = np.arange(m) % 3 if kinds is None else kinds
    u = _directions(rng, kinds)
    p1, c1 = _partner(rng, anchors, u, eps, _cycle_classes(rng, m))
    hinge = np.arange(m) >= n_pairs
    v = _opposed(rng, u, kinds)
    p2, c2 = _partner(rng, anchors[hinge], v[hinge], eps, _cycle_classes(rng, int(hinge.sum())))
    c2_full = np.zeros(m, np.int64)
    c2_full[hinge] = c2
    p2_full = np.zeros_like(anchors)
    p2_full[hinge] = p2
    pts, bonds, bcls, bkind, mol = [], [], [], [], []
    for s in np.nonzero((c1 != 9) & (c2_full != 9))[0]:
        base = len(pts)
        pts += [anchors[s], p1[s]]
        bonds.append((base, base + 1))
        bcls.append(c1[s])
        bkind.append(kinds[s])
        if hinge[s]:
            pts.append(p2_full[s])
            bonds.append((base, base + 2))
            bcls.append(c2_full[s])
            bkind.append(kinds[s])
        mol += [s] * (len(pts) - base)
    return (np.array(pts, F32).reshape(-1, 3), np.array(bonds, np.int64).reshape(-1, 2), np.array(bcls, np.int64),
            np.array(bkind, np.int64), np.array(mol, np.int64))


def _finish(rng, pts, eps, min_samples, bonds, bcls, bkind, mol, **extra):
    """Permute the points and renumber the bookkeeping."""
    n = len(pts)
    assert n <= 30_000
    perm = rng.permutation(n)        # new position i holds old point perm[i]
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    meta = dict(bonds=where[bonds] if len(bonds) else bonds, bond_class=bcls, bond_kind=bkind, molecule=mol[perm],
                source_index=perm, **extra)
    for key in ("groups", "contact", "satellite"):
        if key in meta:
            meta[key] = [where[g] for g in meta[key]] if key == "groups" else where[meta[key]]
    return Case(np.ascontiguousarray(pts[perm]), eps, min_samples, meta)


def _grid_sites(rng, m, half, centre, eps):
    """m distinct sites of the (2 half + 1)^3 grid of spacing 5 eps about centre, jittered, as fp32 anchors."""
    side = 2 * half + 1
    idx = rng.choice(side ** 3, m, replace=False)
    ijk = np.stack([idx % side, idx // side % side, idx // side ** 2], 1) - half
    pos = np.asarray(centre, F64) + float(F32(eps)) * (SITE * ijk + rng.uniform(-JITTER, JITTER, (m, 3)))
    return pos.astype(F32)


THRESHOLD_VARIANTS = {  # eps, centre, grid half width (sites): half extent = 5 eps * half
    "origin": (0.35, (0.0, 0.0, 0.0), 7),          # half extent 12.25
    "offset": (0.35, (37.3, -12.9, 5.1), 7),
    "small_eps": (0.013, (0.3, 0.2, -0.4), 7),     # half extent 0.455
    "large_eps": (2.7, (100.0, -50.0, 25.0), 7),   # half extent 94.5
}


@functools.lru_cache(maxsize=None)
def _threshold_set(variant, seed):
    eps, centre, half = THRESHOLD_VARIANTS[variant]
    rng = np.random.default_rng([seed, sorted(THRESHOLD_VARIANTS).index(variant)])
    anchors = _grid_sites(rng, 2200, half, centre, eps)
    return _molecules(rng, anchors, eps, n_pairs=1200)


def threshold(seed, variant="origin", min_samples=2):
    """Pairs and hinges with every bond at pred(eps2), eps2 or succ(eps2), in the four settings of THRESHOLD_VARIANTS.  All
    three classes are reachable in each of them (a nudge of one ulp of a coordinate moves d2 by 20-180 ulps of eps2 there,
    and 13^3 nudges cover every residue).  min_samples 1 exercises the unions alone, 2 the core count, 3 the border search
    (only the middle of a hinge with two holding bonds is core)."""
    pts, bonds, bcls, bkind, mol = _threshold_set(variant, seed)
    rng = np.random.default_rng([seed, 77])  # (the permutation does not depend on min_samples)
    return _finish(rng, pts, THRESHOLD_VARIANTS[variant][0], min_samples, bonds, bcls, bkind, mol)


def exact_ties(seed, min_samples=2):
    """eps = 0.375 (eps^2 = 0.140625 exactly), points on a 2^-6 lattice out to |x| < 64: every d2 is exact in every form.
    Pairs at exactly eps -- 24 steps along an axis, or (16, 16, 8) steps -- are neighbours (class 0); pairs at 25 steps or
    (16, 16, 9) are not (class +2).  Tells <= from < anywhere in the extent, two cells away along an axis."""
    rng = np.random.default_rng([seed, 101])
    unit, eps, m, half = 2.0 ** -6, 0.375, 2000, 30
    idx = rng.choice((2 * half + 1) ** 3, m, replace=False)
    side = 2 * half + 1
    a = 120 * (np.stack([idx % side, idx // side % side, idx // side ** 2], 1) - half) + rng.integers(-8, 9, (m, 3))
    tie = np.arange(m) % 2 == 0
    axis = np.arange(m) // 2 % 2 == 0
    off = np.zeros((m, 3), np.int64)
    ax = rng.integers(0, 3, m)
    off[np.arange(m), ax] = np.where(tie, 24, 25)
    tri = rng.permuted(np.stack([np.full(m, 16), np.full(m, 16), np.where(tie, 8, 9)], 1), axis=1)
    off = np.where(axis[:, None], off, tri) * rng.choice([-1, 1], (m, 3))
    pts = np.concatenate([a, a + off]).astype(F64) * unit
    assert np.abs(pts).max() < 64
    bonds = np.stack([np.arange(m), np.arange(m) + m], 1)
    mol = np.concatenate([np.arange(m), np.arange(m)])
    return _finish(rng, pts.astype(F32), eps, min_samples, bonds, np.where(tie, 0, 2), np.where(axis, 1, 2), mol)


def blobs(rng, n, eps, centre, centers=4, noise=0.1, spread=0.6, extent=8.0):
    """lattice_blobs (tests/dbscan_reference.py) without the rounding, in units of eps / 0.35, about centre."""
    f = eps / 0.35
    n_noise = int(n * noise)
    c = rng.uniform(-extent, extent, size=(centers, 3))
    which = rng.integers(0, centers, size=n - n_noise)
    pts = np.concatenate([c[which] + rng.normal(0.0, spread, size=(n - n_noise, 3)),
                          rng.uniform(-extent - 2, extent + 2, size=(n_noise, 3))])
    return (np.asarray(centre, F64) + f * pts[rng.permutation(n)]).astype(F32)


FAR = (100.0, -50.0, 25.0)
CLOUDS = {  # name: (n, eps, min_samples, centre, spread)
    "cloud_035_ms5_origin": (10000, 0.35, 5, (0.0, 0.0, 0.0), 0.5),
    "cloud_035_ms10_far": (30000, 0.35, 10, FAR, 0.5),
    "cloud_035_ms600_origin": (20000, 0.35, 600, (0.0, 0.0, 0.0), 0.3),
    "cloud_035_ms600_far": (20000, 0.35, 600, FAR, 0.3),
    "cloud_002_ms5_far": (10000, 0.02, 5, FAR, 0.5),
    "cloud_002_ms10_origin": (30000, 0.02, 10, (0.0, 0.0, 0.0), 0.5),
    "cloud_002_ms600_origin": (20000, 0.02, 600, (0.0, 0.0, 0.0), 0.3),
    "cloud_002_ms600_far": (20000, 0.02, 600, FAR, 0.3),
}


def cloud(seed, name):
    """Gaussian blobs with uniform noise as arbitrary floats: no lattice, at the origin or about (100, -50, 25), with the
    blobs shrunk by eps / 0.35 so that clusters exist at eps = 0.02 too."""
    n, eps, ms, centre, spread = CLOUDS[name]
    rng = np.random.default_rng([seed, sorted(CLOUDS).index(name), 5])
    pts = blobs(rng, n, eps, centre, spread=spread)
    return Case(pts, eps, ms, dict(bonds=np.zeros((0, 2), np.int64)))


STACK_MS = (2, 64, 65, 257)


def stacks(seed, min_samples=64):
    """Stacks of k = min_samples - 1, min_samples, min_samples + 1 points packed within 0.01 eps of a site (one cell, with
    few exceptions; some members are exact duplicates), each with one satellite at a threshold-class distance from the
    stack's first member (the contact).  The other members lie on the side away from the satellite, so the contact and its
    duplicates are the satellite's only possible neighbours and the bond decides between border and noise.  min_samples
    2, 64, 65, 257 straddle the wave and workgroup sizes of the dense-cell shortcut and of the per-wave atomics.  For
    k = min_samples - 1 the satellite decides whether the contact is core."""
    ms = int(min_samples)
    eps = 0.35
    rng = np.random.default_rng([seed, 202, ms])
    per_k = 240 if ms < 64 else (24 if ms < 128 else 12)
    ks = [k for k in (ms - 1, ms, ms + 1) if k >= 1]
    m = per_k * len(ks)
    anchors = _grid_sites(rng, m, 7, (3.3, -7.1, 1.9), eps)
    kinds = np.arange(m) // 3 % 3
    u = _directions(rng, kinds)
    sat, cls = _partner(rng, anchors, u, eps, np.arange(m) % 3 - 1)  # (every k meets every class)
    pts, bonds, bcls, bkind, mol, groups, stack_k = [], [], [], [], [], [], []
    for s in np.nonzero(cls != 9)[0]:
        k = ks[s // per_k]
        base = len(pts)
        t = rng.uniform(-0.01, 0.01, (k - 1, 3)) * eps
        t = np.where((t @ u[s] > 0)[:, None], -t, t)  # on the side away from the satellite
        extra = (anchors[s].astype(F64) + t).astype(F32)
        extra[: (k - 1) // 8] = anchors[s]  # exact duplicates of the contact
        pts += [anchors[s]] + list(extra) + [sat[s]]
        bonds.append((base, base + k))
        bcls.append(cls[s])
        bkind.append(kinds[s])
        groups.append(np.arange(base, base + k))
        stack_k.append(k)
        mol += [s] * (k + 1)
    bonds = np.array(bonds, np.int64)
    return _finish(rng, np.array(pts, F32), eps, ms, bonds, np.array(bcls), np.array(bkind), np.array(mol),
                   groups=groups, stack_k=np.array(stack_k), contact=bonds[:, 0], satellite=bonds[:, 1])


def key_layout(seed, min_samples=2):
    """Molecules along three arms that leave a corner at the origin along x, y and z out to 2.2 * 10^5 (eps = 0.35), so
    that cell indices pass 2^20 on each axis in turn and the 63-bit key cx | cy << 21 | cz << 42 uses its high bits; the y
    arm also has pairs that straddle the multiples of 2^11 cells, where cy crosses the boundary of the two 32-bit words
    the key is sorted by.  A pair at the origin sits in cells 0 and 1 of every axis.  fp32 is coarse out there (one step
    is 0.045 eps): the bonds still reach the threshold classes through their finer coordinates."""
    eps = 0.35
    e = float(F32(eps))
    h = cell_side(eps)
    rng = np.random.default_rng([seed, 303])
    anchors, kinds, is_pair = [np.zeros((1, 3))], [np.array([4])], [np.array([True])]
    for arm in range(3):
        i = np.unique(np.concatenate([rng.integers(6, 121000, 250), rng.integers(121100, 125700, 60)]))
        along = SITE * e * i
        knd = np.arange(len(i)) % 3
        pair = np.arange(len(i)) % 5 < 3
        if arm == 1:  # pairs across the multiples of 2^11 cells: anchor 0.4 eps below, bond along +y
            edge = 2048 * h * np.sort(rng.choice(np.arange(1, 511), 150, replace=False))
            keep = np.abs(along[:, None] - edge[None, :]).min(1) > 6 * e
            along, knd, pair = along[keep], knd[keep], pair[keep]
            along = np.concatenate([along, edge - 0.4 * e])
            knd = np.concatenate([knd, np.full(len(edge), 3)])
            pair = np.concatenate([pair, np.ones(len(edge), bool)])
        pos = 1.0 + e * rng.uniform(-JITTER, JITTER, (len(along), 3))
        pos[:, arm] = along + e * rng.uniform(-JITTER, JITTER, len(along)) * (knd != 3)
        anchors.append(pos)
        kinds.append(knd)
        is_pair.append(pair)
    anchors, kinds, is_pair = np.concatenate(anchors).astype(F32), np.concatenate(kinds), np.concatenate(is_pair)
    order = np.argsort(~is_pair, kind="stable")  # pairs first, as _molecules expects
    anchors, kinds, is_pair = anchors[order], kinds[order], is_pair[order]
    pts, bonds, bcls, bkind, mol = _molecules(rng, anchors, eps, int(is_pair.sum()), kinds=kinds)
    assert pts.min() == 0.0
    return _finish(rng, pts, eps, min_samples, bonds, bcls, bkind, mol)


def axis_limit_x(eps=0.35):
    """(last fp32 X with X / h < 2^21 - 1, the next fp32 value): the widest extent the grid accepts and the first it does
    not, in the arithmetic of the range check (float64 quotient of the fp32 extent by the float64 cell side)."""
    h = cell_side(eps)
    x = F32((2 ** 21 - 1) * h)
    while F64(x) / h >= 2 ** 21 - 1:
        x = np.nextafter(x, F32(0))
    while F64(np.nextafter(x, F32(np.inf))) / h < 2 ** 21 - 1:
        x = np.nextafter(x, F32(np.inf))
    return x, np.nextafter(x, F32(np.inf))


def axis_limit(seed, over=False, min_samples=2):
    """Two pairs, one with a point at x = 0 and one with a point at x = X, the largest coordinate.  With over=False X is the
    last fp32 value the 2^21-cell axis limit accepts: the far pair sits in cells 2^21 - 2 and below, so its +-2 window is
    clamped at the last cell.  With over=True X is the next fp32 value, which must be refused."""
    eps = 0.35
    rng = np.random.default_rng([seed, 404])
    x = axis_limit_x(eps)[1 if over else 0]
    anchors = np.array([[0.0, 0.0, 0.0], [x, 0.1, 0.2]], F32)
    u = _unit(np.array([[0.8, 0.5, 0.33], [-0.9, 0.3, 0.31]]))
    p, cls = _partner(rng, anchors, u, eps, np.array([0, -1]))
    assert (cls != 9).all()
    pts = np.concatenate([anchors, p])
    assert pts[:, 0].min() == 0.0 and pts[:, 0].max() == x
    return _finish(rng, pts, eps, min_samples, np.array([[0, 2], [1, 3]]), cls, np.array([0, 0]), np.array([0, 1, 0, 1]))


def eps_limit(seed, k=-39, min_samples=2):
    """A pair (tie) and a hinge (pred, succ) built for eps = 0.5 with every coordinate in [0.5, 8), so that coordinate
    differences are 0 or at least 2^-24, then scaled by 2^k exactly: k = -39 gives eps = 2^-40 and k = 41 gives eps = 2^40,
    the two ends of the range the exactness argument covers, with no subnormal square and the labels of k = 0."""
    rng = np.random.default_rng([seed, 606])
    anchors = np.array([[1.1, 2.3, 0.7], [5.1, 4.2, 6.3]], F32)
    p1, c1 = _partner(rng, anchors, _unit(np.array([[0.5, -0.6, 0.62], [-0.7, 0.1, 0.7]])), 0.5, np.array([0, -1]))
    p2, c2 = _partner(rng, anchors[1:], _unit(np.array([[0.68, -0.2, -0.7]])), 0.5, np.array([1]))
    assert (c1 != 9).all() and (c2 != 9).all()
    pts = np.ldexp(np.concatenate([anchors, p1, p2]), k).astype(F32)
    return _finish(rng, pts, float(np.ldexp(0.5, k)), min_samples, np.array([[0, 2], [1, 3], [1, 4]]),
                   np.concatenate([c1, c2]), np.zeros(3, np.int64), np.array([0, 1, 0, 1, 1]))


def _even_steps(rng, length, special):
    """Steps of 0.65-0.85 eps (in eps) that add up to length, with steps of 1.0 at the positions listed in special."""
    n = int(round((length - len(special)) / 0.75)) + len(special)
    st = rng.uniform(0.65, 0.85, n)
    st[special] = 1.0
    free = np.ones(n, bool)
    free[special] = False
    st[free] *= (length - len(special)) / st[free].sum()
    return st


CHAIN_FRAME = np.array([[0.8, 0.48, 0.36], [-0.6, 0.64, 0.48], [0.0, -0.6, 0.8]])  # rows e1, e2, e3: orthonormal


def chain(seed, layers=16, rows=16, row_len=60.0, n_special=96, min_samples=2):
    """One filament of more than 20 000 points, consecutive points 0.6-0.9 eps apart, laid as a serpentine in the oblique
    frame CHAIN_FRAME: rows along +e1 and -e1 in turn, 3 eps apart along e2, in layers 3 eps apart along e3 whose rows go
    up and down e2 in turn.  e1 has positive x, y and z parts, so the curve runs with the cell-key order (z, then y, then
    x) in some stretches and against it in others, and it never comes within 2 eps of itself.  n_special links inside the
    rows are threshold bonds along the row (1-4 % across): a third each of succ(eps2) -- the B breaks --, eps2 and
    pred(eps2), which hold.  With min_samples = 2 every point is core and there are B + 1 clusters.  Most points have a
    cell of their own: the unions form the long parent paths that blobs never give the union-find."""
    eps = 0.35
    e = float(F32(eps))
    rng = np.random.default_rng([seed, 505, layers, rows])
    n_rows = layers * rows
    steps_per_row = int(round(row_len / 0.75))
    slots = rng.choice(n_rows * ((steps_per_row - 10) // 5), n_special, replace=False)  # (row, every 5th step from 5 on)
    want = _cycle_classes(rng, n_special)
    pos, special = [np.array([0.0, 0.0, 0.0])], []
    for r in range(n_rows):
        layer, in_layer = divmod(r, rows)
        mine = np.nonzero(slots // ((steps_per_row - 10) // 5) == r)[0]
        at = 5 + 5 * (slots[mine] % ((steps_per_row - 10) // 5))
        st = _even_steps(rng, row_len, at)
        sx = 1.0 if r % 2 == 0 else -1.0
        for k, s in enumerate(st):
            if k in at:
                special.append((len(pos) - 1, want[mine[list(at).index(k)]], sx))
            pos.append(pos[-1] + np.array([sx * s, 0.0, 0.0]))
        if r == n_rows - 1:
            break
        turn = np.array([0.0, 0.0, 0.75]) if in_layer == rows - 1 else np.array([0.0, 0.75 if layer % 2 == 0 else -0.75, 0.0])
        for _ in range(4):
            pos.append(pos[-1] + turn)
    pts = (np.array([-10.3, -8.1, 2.7]) + e * (np.array(pos) @ CHAIN_FRAME)).astype(F32)
    idx = np.array([s[0] for s in special])
    u = np.zeros((len(idx), 3))
    u[:, 0] = [s[2] for s in special]
    u[:, 1:] = rng.uniform(0.01, 0.04, (len(idx), 2)) * rng.choice([-1.0, 1.0], (len(idx), 2))
    p, cls = _partner(rng, pts[idx], _unit(u @ CHAIN_FRAME), eps, np.array([s[1] for s in special]))
    ok = cls != 9
    pts[idx[ok] + 1] = p[ok]
    n = len(pts)
    links = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    bcls = np.full(n - 1, -2, np.int64)
    bcls[idx[ok]] = cls[ok]
    bcls[idx[~ok]] = 2  # (a step of 1.0 eps that no nudge brought to a class: apart, and counted as a break)
    return _finish(rng, pts, eps, min_samples, links, bcls, np.ones(n - 1, np.int64), np.zeros(n, np.int64))


def _registry():
    reg = {}
    for variant in THRESHOLD_VARIANTS:
        for ms in (1, 2, 3):
            reg[f"threshold_{variant}_ms{ms}"] = functools.partial(threshold, variant=variant, min_samples=ms)
    reg["exact_ties_ms1"] = functools.partial(exact_ties, min_samples=1)
    reg["exact_ties_ms2"] = functools.partial(exact_ties, min_samples=2)
    for name in CLOUDS:
        reg[name] = functools.partial(cloud, name=name)
    for ms in STACK_MS:
        reg[f"stacks_ms{ms}"] = functools.partial(stacks, min_samples=ms)
    for ms in (1, 2, 3):
        reg[f"key_layout_ms{ms}"] = functools.partial(key_layout, min_samples=ms)
    reg["axis_limit"] = axis_limit
    reg["eps_limit_lo"] = functools.partial(eps_limit, k=-39)
    reg["eps_limit_hi"] = functools.partial(eps_limit, k=41)
    reg["chain"] = chain
    reg["chain_short"] = functools.partial(chain, layers=4, rows=15)
    return reg


CASES = _registry()
MOLECULE_CASES = [n for n in CASES if n.startswith(("threshold_", "exact_ties", "key_layout", "axis_limit", "eps_limit"))]
STACK_CASES = [n for n in CASES if n.startswith("stacks_")]
SEED = 20260101


@functools.lru_cache(maxsize=None)
def get(name, seed=SEED):
    """The named case (cached: the arrays are read-only)."""
    return CASES[name](seed)
