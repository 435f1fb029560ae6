"""Restatements for goi_hyperplane_amd.field (not collected as a test):

    density_f64            float64 numpy: the density grid of DreamGaussian's extract_fields -- the reference's call sites
                           presuppose it (gui/main.py:607-617) but its tree keeps only gaussian_3d_coeff
                           (gui/gs_renderer.py:66-85) -- with the decisions that are DEFINED in float32 (who is kept, the frame,
                           block membership) taken in float32 and everything else in float64
    density_f32_reference  float32 torch on the CPU, the way the reference would run it: build_scaling_rotation and
                           strip_symmetric, then per block the reference's weight per (point, Gaussian) pair, summed in
                           batches of 1024 Gaussians
    marching_tets          numpy marching tetrahedra on the Kuhn split in the operation order of csrc/field.hip (dtype
                           float32: bit for bit; float64: the restatement of the same surface), its 6 x 16 case table
                           derived here from geometry, not typed in
    extract_mesh_f64       float64: density, iso-surface and the map back to world coordinates
    analytic grids, mesh_topology, outward_fraction: what the tests of the iso-surface share
"""
from __future__ import annotations

import itertools

import numpy as np
import torch

SH_C0 = 0.28209479177387814
EPS32 = float(np.finfo(np.float32).eps)


# ---- the grid ---------------------------------------------------------------------------------------------------------------
def grid_tables(R, num_blocks, relax_ratio, coords=None):
    """coords [R] = torch.linspace(-1, 1, R) and the widened point bounds of every block, (lo, hi) [num_blocks], all float32
    numpy, formed as the reference forms them (vmin -= block_size * relax_ratio on a float32 tensor)."""
    c = torch.linspace(-1, 1, R) if coords is None else torch.as_tensor(np.asarray(coords, dtype=np.float32))
    split = R // num_blocks
    w = (2 / num_blocks) * relax_ratio
    return c.numpy().copy(), (c[0::split] - w).numpy().copy(), (c[split - 1::split] + w).numpy().copy()


def kept_mask(xyz, opacity, min_opacity=0.005, selection=None, selection_invert=False):
    keep = opacity.astype(np.float32) > np.float32(min_opacity)
    if selection is not None:
        keep &= (np.asarray(selection) != 0) != bool(selection_invert)
    return keep & np.isfinite(xyz).all(axis=1)


def frame_f32(xyz, keep, bounds=None):
    """(center float32 [3], scale float32): (amin + amax) / 2 and 1.8 / max extent of the kept centres, as torch rounds them."""
    if bounds is not None:
        return np.asarray(bounds[0], dtype=np.float32).reshape(3), np.float32(bounds[1])
    if not keep.any():
        return np.zeros(3, np.float32), np.float32(1.0)
    mn, mx = xyz[keep].min(axis=0), xyz[keep].max(axis=0)
    ext = np.float32((mx - mn).max())
    return ((mn + mx) / np.float32(2.0)).astype(np.float32), (np.float32(1.8 / float(ext)) if ext > 0 else np.float32(1.0))


def members_f32(cn, keep, lo, hi, bx, by, bz):
    """Indices (ascending) of the Gaussians of block (bx, by, bz): normalised float32 centre strictly inside the bounds."""
    with np.errstate(invalid="ignore"):
        m = keep & (cn[:, 0] > lo[bx]) & (cn[:, 0] < hi[bx]) & (cn[:, 1] > lo[by]) & (cn[:, 1] < hi[by]) \
            & (cn[:, 2] > lo[bz]) & (cn[:, 2] < hi[bz])
    return np.nonzero(m)[0]


def _xp(a):
    return torch if isinstance(a, torch.Tensor) else np


def _columns(a):
    return tuple(a[..., i] for i in range(a.shape[-1]))


def rotation_entries(w, x, y, z):
    """The nine entries, row-major, of the rotation of a unit quaternion (w, x, y, z); numpy or torch."""
    return (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))


def scaled_rotation(scales, quaternions):
    """R(q / |q|) diag(s) as [n, 3, 3], numpy or torch in the dtype of its inputs: column j of the rotation times s_j (the
    product of a matrix with a diagonal one has one non-zero term per entry, so this is what a matmul gives)."""
    xp = _xp(scales)
    w, x, y, z = _columns(quaternions)
    n = xp.sqrt(w * w + x * x + y * y + z * z)
    rot = xp.stack(rotation_entries(w / n, x / n, y / n, z / n), -1).reshape(-1, 3, 3)
    return rot * scales[:, None, :]


def packed_symmetric(S):
    """xx xy xz yy yz zz of [n, 3, 3] symmetric matrices."""
    return _xp(S).stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)


def covariance6(scales, rotation):
    """(R S)(R S)^T packed; numpy or torch (the tests use float64 numpy for the truth, float32 torch for the reference)."""
    L = scaled_rotation(scales, rotation)
    return packed_symmetric(L @ (np.transpose(L, (0, 2, 1)) if isinstance(L, np.ndarray) else L.transpose(1, 2)))


def inverse6(cov):
    """The packed inverse of packed symmetric 3 x 3 matrices by cofactors over det + 1e-24: the regularised inverse the
    reference's weight uses (gui/gs_renderer.py:66-85), in the operation order its pins need; numpy or torch."""
    sxx, sxy, sxz, syy, syz, szz = _columns(cov)
    det = sxx * syy * szz + 2 * syz * sxz * sxy - syz**2 * sxx - sxz**2 * syy - sxy**2 * szz
    r = 1 / (det + 1e-24)
    return ((syy * szz - syz**2) * r, (syz * sxz - sxy * szz) * r, (syz * sxy - sxz * syy) * r,
            (sxx * szz - sxz**2) * r, (sxy * sxz - syz * sxx) * r, (sxx * syy - sxy**2) * r)


def pair_weight(offsets, cov):
    """exp(-d^T inverse6(cov) d / 2) for every row of offsets [..., 3] and packed covariances [..., 6], zero where the
    exponent comes out positive (an indefinite matrix); numpy or torch, in the dtype of its inputs."""
    xp = _xp(offsets)
    dx, dy, dz = _columns(offsets)
    ixx, ixy, ixz, iyy, iyz, izz = inverse6(cov)
    e = -0.5 * (dx**2 * ixx + dy**2 * iyy + dz**2 * izz) - dx * dy * ixy - dx * dz * ixz - dy * dz * iyz
    return xp.exp(xp.where(e > 0, xp.full_like(e, -1e10), e))


def _arrays(model):
    f32 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.float32)  # noqa: E731
    return f32(model["xyz"]), f32(model["opacity"]).reshape(-1), f32(model["scaling"]), f32(model["rotation"])


def density_f64(model, R, num_blocks, relax_ratio=1.5, min_opacity=0.005, selection=None, selection_invert=False,
                attributes=None, bounds=None, coords=None):
    """-> dict(occ [R,R,R], attr [3,R,R,R] or None, opsum [R,R,R] (the sum of the members' opacities at every point),
    members [nb,nb,nb] (counts), center, scale, coords), float64 except the float32 frame and tables."""
    xyz, opacity, scaling, rotation = _arrays(model)
    coords32, lo, hi = grid_tables(R, num_blocks, relax_ratio, coords)
    keep = kept_mask(xyz, opacity, min_opacity, selection, selection_invert)
    center, scale = frame_f32(xyz, keep, bounds)
    with np.errstate(all="ignore"):
        cn32 = (xyz - center) * scale
        keep &= np.isfinite(cn32).all(axis=1)
        cn = (xyz.astype(np.float64) - center.astype(np.float64)) * float(scale)
        cov = covariance6(scaling.astype(np.float64) * float(scale), rotation.astype(np.float64))
    op = opacity.astype(np.float64)
    att = None if attributes is None else np.asarray(attributes, dtype=np.float64)
    split = R // num_blocks
    occ = np.zeros((R, R, R))
    opsum = np.zeros((R, R, R))
    attr = None if att is None else np.zeros((3, R, R, R))
    members = np.zeros((num_blocks,) * 3, dtype=np.int64)
    c64 = coords32.astype(np.float64)
    for bx, by, bz in itertools.product(range(num_blocks), repeat=3):
        idx = members_f32(cn32, keep, lo, hi, bx, by, bz)
        members[bx, by, bz] = idx.size
        if idx.size == 0:
            continue
        sx, sy, sz = (slice(b * split, (b + 1) * split) for b in (bx, by, bz))
        pts = np.stack(np.meshgrid(c64[sx], c64[sy], c64[sz], indexing="ij"), axis=-1).reshape(-1, 3)
        with np.errstate(all="ignore"):
            w = pair_weight(pts[:, None, :] - cn[idx][None, :, :], np.broadcast_to(cov[idx][None], (pts.shape[0], idx.size, 6)))
        ow = w * op[idx][None, :]
        occ[sx, sy, sz] = ow.sum(axis=1).reshape(split, split, split)
        opsum[sx, sy, sz] = op[idx].sum()
        if attr is not None:
            attr[:, sx, sy, sz] = (ow @ att[idx]).T.reshape(3, split, split, split)
    return dict(occ=occ, attr=attr, opsum=opsum, members=members, center=center, scale=scale, coords=coords32)


def density_f32_reference(model, R, num_blocks, relax_ratio=1.5, min_opacity=0.005, selection=None, selection_invert=False,
                          attributes=None, bounds=None, coords=None, batch_g=1024):
    """float32 torch on the CPU as the reference would run extract_fields -> (occ [R,R,R], attr [3,R,R,R] or None) numpy.
    The kept set, the frame and the grid tables are the ones density_f64 uses."""
    xyz, opacity, scaling, rotation = _arrays(model)
    coords32, lo, hi = grid_tables(R, num_blocks, relax_ratio, coords)
    keep = kept_mask(xyz, opacity, min_opacity, selection, selection_invert)
    center, scale = frame_f32(xyz, keep, bounds)
    with np.errstate(all="ignore"):
        keep &= np.isfinite((xyz - center) * scale).all(axis=1)
    k = torch.from_numpy(np.nonzero(keep)[0])
    t = torch.from_numpy
    xyzs = (t(xyz)[k] - t(center)) * float(scale)
    stds = t(scaling)[k] * float(scale)
    opas = t(opacity)[k][None, :]
    covs = covariance6(stds, t(rotation)[k])
    att = None if attributes is None else t(np.ascontiguousarray(np.asarray(attributes), dtype=np.float32))[k]
    split = R // num_blocks
    occ = torch.zeros((R, R, R))
    attr = None if att is None else torch.zeros((3, R, R, R))
    axis = t(coords32)
    tlo, thi = t(lo), t(hi)
    for bx, by, bz in itertools.product(range(num_blocks), repeat=3):
        sl = tuple(slice(b * split, (b + 1) * split) for b in (bx, by, bz))
        pts = torch.stack(torch.meshgrid(axis[sl[0]], axis[sl[1]], axis[sl[2]], indexing="ij"), dim=-1).reshape(-1, 3)
        lo3, hi3 = torch.stack([tlo[bx], tlo[by], tlo[bz]]), torch.stack([thi[bx], thi[by], thi[bz]])
        member = (xyzs < hi3).all(-1) & (xyzs > lo3).all(-1)
        if not member.any():
            continue
        centres, cov, op = xyzs[member], covs[member], opas[:, member]
        n = centres.shape[0]
        offsets = pts[:, None, :].repeat(1, n, 1) - centres[None]  # [points, members, 3], materialised as the torch port does
        cov_rep = cov[None].repeat(pts.shape[0], 1, 1)             # [points, members, 6]
        val, va = 0, 0
        for first in range(0, n, batch_g):
            last = min(first + batch_g, n)
            w = pair_weight(offsets[:, first:last].reshape(-1, 3), cov_rep[:, first:last].reshape(-1, 6)).reshape(pts.shape[0], -1)
            ow = op[:, first:last] * w
            val = val + ow.sum(-1)
            if att is not None:
                va = va + ow @ att[member][first:last]
        occ[sl] = val.reshape(split, split, split)
        if att is not None:
            attr[(slice(None),) + sl] = va.T.reshape(3, split, split, split)
    return occ.numpy(), (None if attr is None else attr.numpy())


def relative_error(x, truth, opsum):
    """max |x - truth| / (|truth| + 64 ulp32 * opsum) over every grid point (opsum broadcasts over attribute channels; the
    attributes of the tests lie in [0, 1], so the same floor serves)."""
    x, truth = np.asarray(x, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    if not np.isfinite(x).all():
        return float("inf")
    return float((np.abs(x - truth) / (np.abs(truth) + 64 * EPS32 * opsum + 1e-300)).max())


# ---- marching tetrahedra ----------------------------------------------------------------------------------------------------
SLOTS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))  # the seven edges a point owns
SLOT_OF = {d: s for s, d in enumerate(SLOTS)}
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic: xyz xzy yxz yzx zxy zyx


def tet_corners(perm):
    """The corners v0 .. v3 of the Kuhn tetrahedron of an axis permutation, as offsets from the cube's origin."""
    v = [np.zeros(3, dtype=np.int64)]
    for axis in perm:
        nxt = v[-1].copy()
        nxt[axis] = 1
        v.append(nxt)
    return v


def _derive_case(corners, m):
    """Triangles of one tetrahedron for the inside mask m (bit k: v_k inside): a list of ((p, q), (p, q), (p, q)) with
    p < q tetrahedron indices naming crossed edges, oriented so that the normal points from inside to outside.  The
    orientation is decided by geometry (edge midpoints), the vertex order is the kernel's: (lone j, lone k, lone l), or
    (ac, ad, bd) and (ac, bd, bc) for two inside vertices a < b against c < d, the last two swapped where needed."""
    ins = [k for k in range(4) if (m >> k) & 1]
    outs = [k for k in range(4) if not (m >> k) & 1]
    if not ins or not outs:
        return []
    e = lambda p, q: (min(p, q), max(p, q))  # noqa: E731
    if len(ins) == 2:
        a, b = ins
        c, d = outs
        tris = [(e(a, c), e(a, d), e(b, d)), (e(a, c), e(b, d), e(b, c))]
    else:
        lone = ins[0] if len(ins) == 1 else outs[0]
        j, k, l = [x for x in range(4) if x != lone]
        tris = [(e(lone, j), e(lone, k), e(lone, l))]
    P = np.array(corners, dtype=np.float64)
    direction = P[outs].mean(axis=0) - P[ins].mean(axis=0)
    out = []
    for tri in tris:
        mid = [(P[p] + P[q]) / 2 for p, q in tri]
        n = np.cross(mid[1] - mid[0], mid[2] - mid[0])
        s = float(n @ direction)
        assert abs(s) > 1e-9
        out.append(tri if s > 0 else (tri[0], tri[2], tri[1]))
    return out


def case_table():
    """[tet][mask] -> triangles as ((owner offset, slot), ...) triples."""
    table = []
    for perm in PERMS:
        corners = tet_corners(perm)
        row = []
        for m in range(16):
            tris = []
            for tri in _derive_case(corners, m):
                tris.append(tuple((tuple(int(x) for x in corners[p]), SLOT_OF[tuple(int(x) for x in corners[q] - corners[p])])
                                  for p, q in tri))
            row.append(tris)
        table.append(row)
    return table


_TABLE = None


def marching_tets(grid, thresh, attr=None, coords=None, dtype=np.float32):
    """-> (vertices [V,3] dtype, faces [F,3] int32, colors [V,3] dtype or None).  grid [X,Y,Z]; inside iff value > thresh;
    vertex = p_a + t (p_b - p_a), t = (thresh - v_a) / (v_b - v_a), a the owner; colour (A_a + t (A_b - A_a)) / thresh; every
    operation rounded to dtype.  Vertices ordered by (owner, slot), faces by (cube, tetrahedron, triangle)."""
    global _TABLE
    if _TABLE is None:
        _TABLE = case_table()
    g = np.asarray(grid).astype(dtype)
    X, Y, Z = g.shape
    th = dtype(thresh)
    with np.errstate(invalid="ignore"):
        inside = g > th
    if coords is None:
        axes = [np.arange(n).astype(dtype) for n in (X, Y, Z)]
    elif isinstance(coords, (tuple, list)):
        axes = [np.asarray(c).astype(dtype) for c in coords]
    else:
        axes = [np.asarray(coords).astype(dtype)] * 3
    N = X * Y * Z
    cross = np.zeros((X, Y, Z, 7), dtype=bool)
    for s, (dx, dy, dz) in enumerate(SLOTS):
        if X - dx < 1 or Y - dy < 1 or Z - dz < 1:
            continue
        cross[:X - dx, :Y - dy, :Z - dz, s] = inside[:X - dx, :Y - dy, :Z - dz] != inside[dx:, dy:, dz:]
    flat = cross.reshape(N * 7)
    index = np.cumsum(flat) - 1  # vertex of (owner, slot) where flat
    owner, slot = np.nonzero(cross.reshape(N, 7))
    ox, oy, oz = np.unravel_index(owner, (X, Y, Z))
    d = np.array(SLOTS, dtype=np.int64)[slot]
    nx, ny, nz = ox + d[:, 0], oy + d[:, 1], oz + d[:, 2]
    va, vb = g[ox, oy, oz], g[nx, ny, nz]
    with np.errstate(all="ignore"):
        t = ((th - va) / (vb - va)).astype(dtype)
        vertices = np.stack([(axes[0][ox] + t * (axes[0][nx] - axes[0][ox])).astype(dtype),
                             (axes[1][oy] + t * (axes[1][ny] - axes[1][oy])).astype(dtype),
                             (axes[2][oz] + t * (axes[2][nz] - axes[2][oz])).astype(dtype)], axis=1).reshape(-1, 3)
        colors = None
        if attr is not None:
            A = np.asarray(attr).astype(dtype)
            aa, ab = A[:, ox, oy, oz], A[:, nx, ny, nz]
            colors = (((aa + t[None] * (ab - aa)).astype(dtype) / th).astype(dtype)).T.reshape(-1, 3)
    faces, keys = [], []
    if X > 1 and Y > 1 and Z > 1:
        lin = np.arange(N).reshape(X, Y, Z)
        cube_lin = lin[:-1, :-1, :-1].reshape(-1)
        for ti, perm in enumerate(PERMS):
            corners = tet_corners(perm)
            m = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
            for k, c in enumerate(corners):
                m |= inside[c[0]:X - 1 + c[0], c[1]:Y - 1 + c[1], c[2]:Z - 1 + c[2]].astype(np.int64) << k
            m = m.reshape(-1)
            for case in range(1, 15):
                sel = np.nonzero(m == case)[0]
                if sel.size == 0:
                    continue
                origin = cube_lin[sel]
                for k, tri in enumerate(_TABLE[ti][case]):
                    f = np.stack([index[(origin + (off[0] * Y + off[1]) * Z + off[2]) * 7 + s] for off, s in tri], axis=1)
                    faces.append(f)
                    keys.append(np.stack([origin, np.full(sel.size, ti), np.full(sel.size, k)], axis=1))
    if faces:
        faces, keys = np.concatenate(faces), np.concatenate(keys)
        order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        faces = faces[order].astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    return vertices, faces, colors


def extract_mesh_f64(model, density_thresh=1.0, R=128, num_blocks=16, relax_ratio=1.5, colors=None, **kw):
    """float64: density, iso-surface, v / scale + center, colours clamped -> (vertices, faces, colors, center, scale)."""
    f = density_f64(model, R, num_blocks, relax_ratio, attributes=colors, **kw)
    v, faces, c = marching_tets(f["occ"], density_thresh, f["attr"], f["coords"].astype(np.float64), dtype=np.float64)
    v = v / float(f["scale"]) + f["center"].astype(np.float64)
    return v, faces, (None if c is None else np.clip(c, 0.0, 1.0)), f["center"], f["scale"]


# ---- analytic grids and mesh checks -----------------------------------------------------------------------------------------
def _points(shape):
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)


def sphere_grid(shape=(16, 16, 16), center=(7.3, 7.6, 7.1), radius=5.2):
    """(grid float32, thresh): value 2 - |p - c| / r, inside (> 1) the ball."""
    p = _points(shape)
    return (2.0 - np.linalg.norm(p - np.array(center), axis=-1) / radius).astype(np.float32), 1.0


def torus_grid(shape=(24, 24, 12), center=(11.4, 11.7, 5.3), major=7.1, minor=2.6):
    p = _points(shape) - np.array(center)
    q = np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - major) ** 2 + p[..., 2] ** 2)
    return (2.0 - q / minor).astype(np.float32), 1.0


def two_spheres_grid(shape=(24, 14, 13)):
    a, _ = sphere_grid(shape, (5.3, 6.6, 6.1), 3.7)
    b, _ = sphere_grid(shape, (17.2, 6.9, 6.4), 4.1)
    return np.maximum(a, b), 1.0


def plane_grid(shape=(12, 14, 13), normal=(0.3137, 0.5219, 0.8043), offset=9.4131):
    p = _points(shape)
    return (1.0 + (offset - p @ np.array(normal)) / 4.0).astype(np.float32), 1.0


def noisy_grid(shape=(40, 40, 40), seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 2.0, size=shape).astype(np.float32), 1.0


def equal_grid(shape=(12, 12, 12)):
    """Small integers with many points exactly at the threshold (outside by the rule value > thresh)."""
    p = _points(shape)
    r = np.abs(p - 5.0).max(axis=-1)  # a cube of Chebyshev radius
    return (4.0 - np.floor(r)).astype(np.float32), 2.0  # values 4, 3 inside; 2 (== thresh) and below outside


def grid_attributes(shape, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.5, size=(3,) + tuple(shape)).astype(np.float32)


def mesh_topology(faces, n_vertices):
    """dict(chi = V - E + F, edge_use = {uses: number of edges}, boundary_edges [B,2], consistent = every interior edge is
    walked once in each direction)."""
    f = np.asarray(faces, dtype=np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(d, axis=1)
    uniq, inv, cnt = np.unique(und, axis=0, return_inverse=True, return_counts=True)
    sign = np.where(d[:, 0] < d[:, 1], 1, -1)
    balance = np.bincount(inv.reshape(-1), weights=sign, minlength=len(uniq))
    used = np.unique(f).size
    return dict(chi=int(used - len(uniq) + len(f)), edge_use={int(k): int((cnt == k).sum()) for k in np.unique(cnt)},
                boundary_edges=uniq[cnt == 1], consistent=bool(np.all(balance[cnt == 2] == 0)), used_vertices=int(used),
                all_used=bool(used == n_vertices))


def face_normals(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3.0


def sphere_shell_model(P=2000, radius=0.8, seed=0, sigma=0.4, opacity=0.6):
    """P nearly isotropic Gaussians on a sphere shell (Fibonacci lattice) with sigma = radius / 2: the density of a uniformly
    covered shell at distance d from its centre is P opacity (sigma^2 / (2 d r)) (exp(-(d - r)^2 / 2 sigma^2) -
    exp(-(d + r)^2 / 2 sigma^2)): 0.135 P opacity at the centre, 0.149 at r / 2, 0.125 on the shell and falling outside.
    "thresh" is its value ON the shell, so the surface density == thresh is the shell itself and the inside is solid.  (With
    num_blocks = 2 and relax_ratio = 1.5 every block holds every Gaussian, so the grid has that profile.)"""
    rng = np.random.default_rng(seed)
    i = np.arange(P) + 0.5
    phi = np.arccos(1 - 2 * i / P)
    th = np.pi * (1 + 5 ** 0.5) * i
    d = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    center = np.array([0.4, -0.3, 1.1])
    thresh = P * opacity * (sigma ** 2 / (2 * radius ** 2)) * (1 - np.exp(-2 * radius ** 2 / sigma ** 2))
    return dict(xyz=(radius * d + center).astype(np.float32), opacity=np.full(P, opacity, np.float32),
                scaling=(sigma * rng.uniform(0.95, 1.05, size=(P, 3))).astype(np.float32),
                rotation=rng.normal(size=(P, 4)).astype(np.float32), rgb=rng.uniform(0, 1, size=(P, 3)).astype(np.float32),
                shell_center=center, shell_radius=radius, thresh=float(thresh))


# ---- the density cases of tests/test_gpu_field.py ---------------------------------------------------------------------------
def _gaussians(rng, n):
    """n Gaussians without centres: normalised scales >= 0.02, anisotropy <= 10 : 1, quaternions of any norm, opacities well
    above the cut."""
    smin = rng.uniform(0.02, 0.04, size=(n, 1))
    fac = rng.uniform(1.0, 10.0, size=(n, 3))
    fac[np.arange(n), rng.integers(0, 3, size=n)] = 1.0
    return dict(opacity=rng.uniform(0.05, 1.0, size=n).astype(np.float32), scaling=(smin * fac).astype(np.float32),
                rotation=(rng.normal(size=(n, 4)) * np.exp(rng.normal(size=(n, 1)))).astype(np.float32))


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def cluster_case(coords, R, num_blocks, relax_ratio, counts, seed):
    """A model in the frame (center 0, scale 1) -- to be run with bounds=(zeros(3), 1.0) -- whose Gaussians sit in the CORE of
    chosen blocks (the part of a block's widened bounds that no other block claims; needs relax_ratio < 0.45), so that block
    (bx, by, bz) has exactly counts[(bx, by, bz)] members, plus Gaussians that must contribute nothing: opacities below the cut
    and one exactly at it, a NaN and an infinite centre, and centres exactly on the outer widened bounds."""
    assert relax_ratio < 0.45
    rng = np.random.default_rng(seed)
    _, lo, hi = grid_tables(R, num_blocks, relax_ratio, coords)
    bs = 2.0 / num_blocks

    def core(b, n):
        return rng.uniform((b + relax_ratio + 0.05) * bs - 1.0, (b + 1 - relax_ratio - 0.05) * bs - 1.0, size=n)
    parts = []
    for (bx, by, bz), n in counts.items():
        g = _gaussians(rng, n)
        g["xyz"] = np.stack([core(bx, n), core(by, n), core(bz, n)], axis=1).astype(np.float32)
        parts.append(g)
    (bx, by, bz) = max(counts, key=counts.get)
    dead = _gaussians(rng, 12)  # in the core of the fullest block, all excluded
    dead["xyz"] = np.stack([core(bx, 12), core(by, 12), core(bz, 12)], axis=1).astype(np.float32)
    dead["opacity"][:6] = rng.uniform(0.0, 0.0049, size=6).astype(np.float32)
    dead["opacity"][6] = np.float32(0.005)  # exactly the cut: excluded by the strict comparison
    dead["xyz"][7, 1] = np.nan
    dead["xyz"][8, 2] = np.inf
    dead["xyz"][9, 0] = lo[0]                 # on the outer widened bounds: the strict test excludes them
    dead["xyz"][10, 1] = hi[num_blocks - 1]
    dead["xyz"][11, 2] = lo[0]
    dead["opacity"][7:] = 0.9
    parts.append(dead)
    m = _cat(parts)
    perm = rng.permutation(len(m["opacity"]))
    m = {k: v[perm] for k, v in m.items()}
    m["rgb"] = rng.uniform(0.0, 1.0, size=(len(perm), 3)).astype(np.float32)
    return m


def random_case(P, seed, spread=(1.0, 0.7, 0.4)):
    """P Gaussians in a box of the given half extents about an off-centre point, scales such that the NORMALISED ones
    (scale 1.8 / 2 spread[0]) stay >= 0.02; a few below the opacity cut, one at it, a NaN and an infinite centre."""
    rng = np.random.default_rng(seed)
    g = _gaussians(rng, P)
    g["scaling"] = (g["scaling"] * (2 * spread[0] / 1.8)).astype(np.float32)
    g["xyz"] = (rng.uniform(-1, 1, size=(P, 3)) * np.array(spread) + np.array([3.0, -2.0, 0.5])).astype(np.float32)
    g["opacity"][:5] = rng.uniform(0.0, 0.0049, size=5).astype(np.float32)
    g["opacity"][5] = np.float32(0.005)
    g["xyz"][6, 0] = np.nan
    g["xyz"][7, 1] = -np.inf
    g["rgb"] = rng.uniform(0.0, 1.0, size=(P, 3)).astype(np.float32)
    return g


# ---- the block loop in torch on any device (tools/field_time.py times it against the kernel) --------------------------------
def density_torch_blockloop(xyz, opacity, scaling, rotation, R=128, num_blocks=16, relax_ratio=1.5, min_opacity=0.005,
                            batch_g=1024, block_stride=1):
    """extract_fields as the reference's port would run it, on the device of its inputs (float32 torch tensors): the kept
    Gaussians index-selected, normalised, their covariances built, then one host-side iteration per block that masks the
    members, materialises the [points, members, 3] offsets and [points, members, 6] covariances and sums the pair weights
    in batches of batch_g Gaussians.  block_stride > 1 visits only every block_stride-th block (for timing a sample).
    -> (occ [R, R, R], blocks visited)."""
    dev = xyz.device
    mask = opacity.reshape(-1) > min_opacity
    opas = opacity.reshape(-1)[mask][None, :]
    xyzs, stds = xyz[mask], scaling[mask]
    mn, mx = xyzs.amin(0), xyzs.amax(0)
    center = (mn + mx) / 2
    scale = 1.8 / (mx - mn).amax().item()
    xyzs = (xyzs - center) * scale
    stds = stds * scale
    covs = covariance6(stds, rotation[mask])
    occ = torch.zeros((R, R, R), dtype=torch.float32, device=dev)
    widen = (2 / num_blocks) * relax_ratio
    split = R // num_blocks
    axis = torch.linspace(-1, 1, R, device=dev)
    visited = 0
    for n, (bx, by, bz) in enumerate(itertools.product(range(num_blocks), repeat=3)):
        if n % block_stride:
            continue
        visited += 1
        sl = tuple(slice(b * split, (b + 1) * split) for b in (bx, by, bz))
        pts = torch.stack(torch.meshgrid(axis[sl[0]], axis[sl[1]], axis[sl[2]], indexing="ij"), dim=-1).reshape(-1, 3)
        lo3, hi3 = pts.amin(0) - widen, pts.amax(0) + widen
        member = (xyzs < hi3).all(-1) & (xyzs > lo3).all(-1)
        if not member.any():
            continue
        centres, cov, op = xyzs[member], covs[member], opas[:, member]
        count = centres.shape[0]
        offsets = pts[:, None, :].repeat(1, count, 1) - centres[None]
        cov_rep = cov[None].repeat(pts.shape[0], 1, 1)
        val = 0
        for first in range(0, count, batch_g):
            last = min(first + batch_g, count)
            w = pair_weight(offsets[:, first:last].reshape(-1, 3), cov_rep[:, first:last].reshape(-1, 6)).reshape(pts.shape[0], -1)
            val = val + (op[:, first:last] * w).sum(-1)
        occ[sl] = val.reshape(split, split, split)
    return occ, visited
