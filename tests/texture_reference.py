"""numpy restatement of goi_hyperplane_amd/texture.py (csrc/texture.hip): float32, one rounding per operation, in the order the
module's docstring writes down, so that the device's results can be compared bit for bit.  Also the shared inputs of
tests/golden/make_texture_golden.py, tests/test_texture_cpu.py and tests/test_gpu_texture.py (grid-put samples, fill masks)
and a float64 grid put for the error gate.  No GPU, no torch."""
from __future__ import annotations

import functools
import math

import numpy as np

F32 = np.float32
ONE, HALF, TWO = F32(1), F32(0.5), F32(2)
MAX_SCREEN = F32(1048576.0)
WAVE_PIXELS = 1024  # csrc/texture.hip's TEX_WAVE_PIXELS: a larger clipped box takes the rasterizer's second path


# ---- atlas ------------------------------------------------------------------------------------------------------------------
def atlas_grid(F, size):
    pairs = (F + 1) // 2
    n = math.isqrt(pairs - 1) + 1 if pairs > 0 else 1
    cell = size // n
    if cell < 4:
        raise ValueError("a cell under 4 texels")
    return n, cell


def atlas(F, size):
    """-> vt float32 [3 F, 2], ft int32 [F, 3], texel float64 [F, 3, 2] (the corners in texel units), (n, cell)"""
    n, cell = atlas_grid(F, size)
    f = np.arange(F, dtype=np.int64)
    p = f // 2
    origin = np.stack([cell * (p % n), cell * (p // n)], axis=1).astype(np.float64)
    c = float(cell)
    lower = np.array([[0.5, 0.5], [c - 2.5, 0.5], [0.5, c - 2.5]])
    upper = np.array([[c - 1.5, c - 1.5], [1.5, c - 1.5], [c - 1.5, 1.5]])
    texel = np.where((f % 2 == 1)[:, None, None], upper[None], lower[None]) + origin[:, None, :]
    vt = (texel.astype(F32) / F32(size - 1)).reshape(3 * F, 2)
    return vt, np.arange(3 * F, dtype=np.int32).reshape(F, 3), texel, (n, cell)


# ---- cameras ----------------------------------------------------------------------------------------------------------------
def clip_positions(v, m):
    v, m = np.asarray(v, F32), np.asarray(m, F32)
    return ((v[:, 0:1] * m[0] + v[:, 1:2] * m[1]) + v[:, 2:3] * m[2]) + m[3]


# ---- rasterize --------------------------------------------------------------------------------------------------------------
def _enc(zw):
    u = np.ascontiguousarray(zw, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _setup(vc, idx, H, W):
    V = len(vc)
    if any(i < 0 or i >= V for i in idx):
        return None
    p = vc[list(idx)]
    w, z = p[:, 3], p[:, 2]
    if not np.all(w > 0):
        return None
    with np.errstate(all="ignore"):
        sx = ((p[:, 0] / w + ONE) * F32(W) - ONE) * HALF
        sy = ((p[:, 1] / w + ONE) * F32(H) - ONE) * HALF
    if not (np.all(np.abs(sx) <= MAX_SCREEN) and np.all(np.abs(sy) <= MAX_SCREEN)):
        return None
    X = np.rint(sx * F32(256)).astype(np.int64)
    Y = np.rint(sy * F32(256)).astype(np.int64)
    a2 = int((X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]))
    if a2 == 0:
        return None
    x0, x1 = max(0, int((X.min() + 255) >> 8)), min(W - 1, int(X.max() >> 8))
    y0, y1 = max(0, int((Y.min() + 255) >> 8)), min(H - 1, int(Y.max() >> 8))
    return X, Y, z, w, abs(a2), (1 if a2 > 0 else -1), x0, x1, y0, y1


def rasterize(v_clip, faces, H, W, info=None):
    """-> tri int32 [H, W], bary float32 [H, W, 2], zw float32 [H, W].  info (a dict): "large" = the faces whose clipped box
    holds more than WAVE_PIXELS pixels, "covered" [F] = the pixels each face covers (before the depth test)."""
    vc = np.ascontiguousarray(v_clip, F32).reshape(-1, 4)
    key = np.full((H, W), np.iinfo(np.uint64).max, np.uint64)
    tri = np.zeros((H, W), np.int32)
    bary = np.zeros((H, W, 2), F32)
    zw_out = np.zeros((H, W), F32)
    large, covered = [], np.zeros(len(faces), np.int64)
    for f, idx in enumerate(np.asarray(faces).tolist()):
        s = _setup(vc, idx, H, W)
        if s is None:
            continue
        X, Y, z, w, area, sgn, x0, x1, y0, y1 = s
        if x1 < x0 or y1 < y0:
            continue
        if (x1 - x0 + 1) * (y1 - y0 + 1) > WAVE_PIXELS:
            large.append(f)
        px, py = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64), np.arange(y0, y1 + 1, dtype=np.int64))
        cover = np.ones(px.shape, bool)
        e = []
        for k in range(3):
            a, b = (k + 1) % 3, (k + 2) % 3
            dx, dy = int(X[b] - X[a]) * sgn, int(Y[b] - Y[a]) * sgn
            ek = dx * (256 * py - int(Y[a])) - dy * (256 * px - int(X[a]))
            cover &= (ek > 0) | ((ek == 0) & (dy > 0 or (dy == 0 and dx < 0)))
            e.append(ek)
        covered[f] = int(cover.sum())
        with np.errstate(all="ignore"):
            A = F32(area)
            s0, s1, s2 = (ek.astype(F32) / A for ek in e)
            p0, p1, p2 = s0 / w[0], s1 / w[1], s2 / w[2]
            tot = (p0 + p1) + p2
            u, v = p0 / tot, p1 / tot
            r = (ONE - u) - v
            zi = (u * z[0] + v * z[1]) + r * z[2]
            wi = (u * w[0] + v * w[1]) + r * w[2]
            zw = zi / wi
        k64 = (_enc(zw).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        sub = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        win = cover & ~np.isnan(zw) & (k64 < key[sub])
        key[sub] = np.where(win, k64, key[sub])
        tri[sub] = np.where(win, f + 1, tri[sub])
        zw_out[sub] = np.where(win, zw, zw_out[sub])
        bary[sub] = np.where(win[..., None], np.stack([u, v], axis=-1), bary[sub])
    if info is not None:
        info["large"], info["covered"] = large, covered
    return tri, bary, zw_out


# ---- resolve ----------------------------------------------------------------------------------------------------------------
def resolve(tri, bary, vt, ft, vn, faces, pose_rot, image, info=None):
    """-> coords float32 [HW, 2], values float32 [HW, 3], valid bool [HW].  info: "viewcos" and "uv" (before the clamp) [HW]."""
    H, W = tri.shape
    t = tri.reshape(-1)
    hit = t > 0
    f = np.where(hit, t - 1, 0)
    u, v = bary.reshape(-1, 2)[:, 0], bary.reshape(-1, 2)[:, 1]
    r = (ONE - u) - v
    vt, vn, R = np.asarray(vt, F32), np.asarray(vn, F32), np.asarray(pose_rot, F32)

    def interp(attr, tris):
        a0, a1, a2 = attr[tris[f, 0]], attr[tris[f, 1]], attr[tris[f, 2]]
        return (u[:, None] * a0 + v[:, None] * a1) + r[:, None] * a2
    if len(faces) == 0:
        uv, n = np.zeros((H * W, 2), F32), np.zeros((H * W, 3), F32)
    else:
        uv, n = interp(vt, np.asarray(ft)), interp(vn, np.asarray(faces))
    dot = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    n = n / np.sqrt(np.maximum(dot, F32(1e-20)))[:, None]
    viewcos = (n[:, 0] * R[0, 2] + n[:, 1] * R[1, 2]) + n[:, 2] * R[2, 2]
    valid = hit & (viewcos > HALF)
    cl = np.minimum(np.maximum(uv, F32(0)), ONE)
    coords = np.where(hit[:, None], np.stack([cl[:, 1] * TWO - ONE, cl[:, 0] * TWO - ONE], axis=1), F32(0)).astype(F32)
    values = np.ascontiguousarray(np.asarray(image, F32).reshape(3, -1).T)
    if info is not None:
        info["viewcos"], info["uv"] = np.where(hit, viewcos, np.nan), np.where(hit[:, None], uv, np.nan)
    return coords, values, valid


# ---- grid put ---------------------------------------------------------------------------------------------------------------
def linear_put(cH, cW, coords, values, valid=None, dtype=F32):
    """linear_grid_put_2d(return_count=True): every texel sums its taps in (tap 00 01 10 11, sample) order."""
    T = dtype
    co, va = np.asarray(coords, F32).astype(T), np.asarray(values, F32).astype(T)
    C = va.shape[1]
    ok = np.isfinite(co).all(axis=1) if len(co) else np.zeros(0, bool)
    if valid is not None:
        ok &= np.asarray(valid, bool)
    co, va = co[ok], va[ok]
    fi = (co[:, 0] * T(0.5) + T(0.5)) * T(cH - 1)
    fj = (co[:, 1] * T(0.5) + T(0.5)) * T(cW - 1)
    i0 = np.clip(np.floor(fi), 0, cH - 2)
    j0 = np.clip(np.floor(fj), 0, cW - 2)
    h, w = fi - i0.astype(T), fj - j0.astype(T)
    i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
    res, cnt = np.zeros((cH * cW, C), T), np.zeros(cH * cW, T)
    for tap in range(4):
        wt = (h if tap & 2 else T(1) - h) * (w if tap & 1 else T(1) - w)
        idx = (i0 + (tap >> 1)) * cW + j0 + (tap & 1)
        np.add.at(res, idx, va * wt[:, None])
        np.add.at(cnt, idx, wt)
    return res.reshape(cH, cW, C), cnt.reshape(cH, cW)


def _lerp_index(out, n_in, T):
    scale = T(n_in) / T(out)
    src = np.maximum(scale * (np.arange(out).astype(T) + T(0.5)) - T(0.5), T(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(T)
    return i0, i1, T(1) - l1, l1


def upsample(level, H, W, dtype=F32):
    """upsample_bilinear2d(align_corners=False) of [cH, cW, C] to [H, W, C]."""
    T = dtype
    y0, y1, hy0, hy1 = _lerp_index(H, level.shape[0], T)
    x0, x1, wx0, wx1 = _lerp_index(W, level.shape[1], T)
    g = lambda y, x: level[y[:, None], x[None, :]]  # noqa: E731
    a0, a1 = wx0[None, :, None], wx1[None, :, None]
    top = a0 * g(y0, x0) + a1 * g(y0, x1)
    bot = a0 * g(y1, x0) + a1 * g(y1, x1)
    return hy0[:, None, None] * top + hy1[:, None, None] * bot


def levels(H, W, min_resolution):
    out = []
    while min(H, W) > min_resolution:
        out.append((H, W))
        H, W = H // 2, W // 2
    return out


def grid_put(H, W, coords, values, valid=None, min_resolution=32, dtype=F32):
    """mipmap_linear_grid_put_2d(return_count=True) without the early exit -> result [H, W, C], count [H, W]."""
    C = np.asarray(values).shape[1]
    result, count = np.zeros((H, W, C), dtype), np.zeros((H, W), dtype)
    for cH, cW in levels(H, W, min_resolution):
        hole = count == 0
        res, cnt = linear_put(cH, cW, coords, values, valid, dtype)
        result = np.where(hole[..., None], result + upsample(res, H, W, dtype), result)
        count = np.where(hole, count + upsample(cnt[..., None], H, W, dtype)[..., 0], count)
    return result, count


def accumulate(albedo, cnt, cur, cur_cnt):
    take = cnt < F32(0.1)
    return np.where(take[..., None], albedo + cur, albedo), np.where(take, cnt + cur_cnt, cnt)


def normalize(albedo, cnt):
    mask = cnt > 0
    with np.errstate(all="ignore"):
        return np.where(mask[..., None], albedo / np.where(mask, cnt, ONE)[..., None], albedo), mask


# ---- fill -------------------------------------------------------------------------------------------------------------------
def fill_nearest(mask, radius=32):
    """-> nearest int32 [h, w]: for a texel outside the mask with a mask texel within L1 distance `radius`, the flat index of the
    mask texel with the smallest (dx^2 + dy^2, row, column); -1 elsewhere.  d2 int64 [h, w] (-1 elsewhere).  Brute force over
    the (2 radius + 1)^2 window, one shift at a time."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    big = np.iinfo(np.int64).max
    best = np.full((h, w), big, np.int64)
    region = np.zeros((h, w), bool)
    rows, cols = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
            yt, xt = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
            m = mask[yt, xt]  # the texel at (y + dy, x + dx) seen from (y, x)
            if not m.any():
                continue
            k = (np.int64(dy * dy + dx * dx) << 42) | (rows[yt, xt] << 21) | cols[yt, xt]
            best[ys, xs] = np.where(m, np.minimum(best[ys, xs], k), best[ys, xs])
            if abs(dy) + abs(dx) <= radius:
                region[ys, xs] |= m
    region &= ~mask
    near = np.where(region, ((best >> 21) & 0x1FFFFF) * w + (best & 0x1FFFFF), -1).astype(np.int32)
    return near, np.where(region, best >> 42, -1)


def fill(albedo, mask, radius=32):
    near, _ = fill_nearest(mask, radius)
    flat = np.asarray(albedo, F32).reshape(-1, albedo.shape[-1])
    src = np.where(near.reshape(-1) >= 0, near.reshape(-1), np.arange(flat.shape[0]))
    return flat[src].reshape(albedo.shape), near


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
PUT_H = PUT_W = 64
PUT_MIN_RESOLUTION = 16  # levels 64 and 32
PUT_SIZES = (0, 1, 5000)


@functools.lru_cache(maxsize=None)
def put_case(N):
    """coords float32 [N, 2], values float32 [N, 3], valid bool [N].  N = 5000: uniform samples (a few a little outside
    [-1, 1]), coordinates of exactly -1 and +1 in every combination, 2000 samples inside one texel, and a mask that removes a
    third of the samples."""
    rng = np.random.default_rng(1000 + N)
    coords = rng.uniform(-1.02, 1.02, size=(N, 2)).astype(F32)
    values = rng.uniform(0, 1, size=(N, 3)).astype(F32)
    valid = np.ones(N, bool)
    if N >= 5000:
        coords[:8] = np.array([[-1, -1], [-1, 1], [1, -1], [1, 1], [-1, 0.3], [0.3, -1], [1, -0.7], [-0.7, 1]], F32)
        centre = (np.array([20.5, 41.5]) / (PUT_H - 1) * 2 - 1)
        coords[1000:3000] = (centre + rng.uniform(-0.4, 0.4, size=(2000, 2)) * 2 / (PUT_H - 1)).astype(F32)
        valid = (np.arange(N) % 3) != 1
        valid[:8] = True
    for a in (coords, values, valid):
        a.setflags(write=False)
    return coords, values, valid


def views_case(h=32, w=32, seed=7):
    """Three synthetic (cur_albedo [h, w, 3], cur_cnt [h, w]) views for accumulate: the first reaches the left two thirds
    (some counts under 0.1), the second the right two thirds, the third everything."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(3):
        cnt = rng.uniform(0.0, 2.0, size=(h, w)).astype(F32)
        cnt[rng.uniform(size=(h, w)) < 0.2] *= F32(0.04)  # counts under 0.1: the next view still adds
        if k == 0:
            cnt[:, 2 * w // 3:] = 0
        if k == 1:
            cnt[:, : w // 3] = 0
        alb = (rng.uniform(0, 1, size=(h, w, 3)).astype(F32) * cnt[..., None]).astype(F32)
        out.append((alb, cnt))
    return out


FILL_SIZE = 96
FILL_RADIUS = 32


@functools.lru_cache(maxsize=None)
def fill_masks():
    """The 96 x 96 masks of the fill tests, by name."""
    n = FILL_SIZE
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    disc = lambda cy, cx, r: (y - cy) ** 2 + (x - cx) ** 2 <= r * r  # noqa: E731
    border = np.zeros((n, n), bool)
    border[0:9, 5:40] = True
    border[60:64, 90:96] = True
    rng = np.random.default_rng(3)
    boxes = np.zeros((n, n), bool)
    for _ in range(6):
        y0, x0 = rng.integers(0, n - 12, size=2)
        hh, ww = rng.integers(2, 12, size=2)
        boxes[y0:y0 + hh, x0:x0 + ww] = True
    single = np.zeros((n, n), bool)
    single[37, 58] = True
    masks = {"disc": disc(50, 45, 11), "two": disc(30, 28, 7) | disc(66, 70, 9), "border": border, "boxes": boxes,
             "single": single, "empty": np.zeros((n, n), bool), "full": np.ones((n, n), bool)}
    for m in masks.values():
        m.setflags(write=False)
    return masks


def fill_albedo(seed=11):
    return np.random.default_rng(seed).uniform(0, 1, size=(FILL_SIZE, FILL_SIZE, 3)).astype(F32)


# ---- rasterizer inputs ------------------------------------------------------------------------------------------------------
def _clip(points, H, W, w=None):
    """Screen positions (sx, sy, depth) -> clip-space rows (x, y, z, w) with ndc = (2 s + 1) / size - 1."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    w = np.ones(len(p)) if w is None else np.asarray(w, np.float64)
    ndc = np.stack([(2 * p[:, 0] + 1) / W - 1, (2 * p[:, 1] + 1) / H - 1, p[:, 2]], axis=1)
    return np.concatenate([ndc * w[:, None], w[:, None]], axis=1).astype(F32)


def hand_cases(H, W):
    """name -> (v_clip float32 [V, 4], faces int32 [F, 3]); positions are given in pixels (they need min(H, W) >= 45)."""
    tris = lambda n: np.arange(3 * n, dtype=np.int32).reshape(n, 3)  # noqa: E731
    c = {}
    # two triangles sharing the diagonal (4, 4) - (40, 40), which runs through pixel centres.  The fill rule gives it to the
    # second; the first is nearer, so a pixel that both covered would show the first
    c["shared_edge"] = (_clip([[4, 4, .4], [40, 4, .4], [40, 40, .4], [4, 4, .5], [40, 40, .5], [4, 40, .5]], H, W), tris(2))
    c["coplanar"] = (_clip([[5, 6, .5], [33, 9, .5], [12, 38, .5]] * 2, H, W), tris(2))
    c["full_frame"] = (_clip([[-10, -10, .7], [3 * W, -10, .7], [-10, 3 * H, .7]], H, W, w=[1.0, 2.5, 0.7]), tris(1))
    c["sliver"] = (_clip([[10.2, 10.3, .5], [30.7, 10.4, .5], [20.1, 10.35, .5]], H, W), tris(1))
    c["half_off"] = (_clip([[-20, 10, .5], [20, 12, .3], [-5, 40, .6]], H, W, w=[1.0, 2.0, 3.0]), tris(1))
    c["w_nonpositive"] = (_clip([[5, 5, .5], [30, 5, .5], [5, 30, .5], [6, 6, .5], [31, 6, .5], [6, 31, .5]], H, W,
                                w=[1, 1, 1, 1, -1, 1]), tris(2))
    c["zero_area"] = (_clip([[5, 5, .5], [15, 15, .5], [25, 25, .5], [7, 7, .5], [7, 7, .5], [20, 9, .5]], H, W), tris(2))
    c["back_facing"] = (_clip([[8, 8, .5], [10, 36, .5], [36, 12, .5]], H, W), tris(1))
    vs, fs, off = [], [], 0
    for v, f in c.values():
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    c["all"] = (np.concatenate(vs), np.concatenate(fs).astype(np.int32))
    c["no_faces"] = (c["coplanar"][0], np.zeros((0, 3), np.int32))
    return c


@functools.lru_cache(maxsize=None)
def unit_mesh(name):
    """The named iso-surface of tests/mesh_reference.py moved to the origin and scaled into the unit ball, with vertex
    normals: (vertices float32 [V, 3], faces int32 [F, 3], normals float32 [V, 3])."""
    from tests import mesh_reference
    v, f, _ = mesh_reference.grid_mesh(name)
    lo, hi = v.min(axis=0), v.max(axis=0)
    v = ((v - (lo + hi) * F32(0.5)) / F32(0.75 * float((hi - lo).max()))).astype(F32)
    out = (v, f.copy(), mesh_reference.vertex_normals(v, f))
    for a in out:
        a.setflags(write=False)
    return out
