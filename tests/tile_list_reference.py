"""Plain float64 reference of which (tile, Gaussian) pairs a culled tile list MUST hold and which it MAY NOT hold.

TEST INFRASTRUCTURE ONLY (numpy).  It models none of the kernel's arithmetic (no outward roundings, no Kahan determinant,
no tile masks): it takes the oracle's forward state -- means2D, conic_opacity, depths, point_list, ranges, all fp32 and all
asserted bit-equal to the device's at cull_variant 0 by the GPU tests -- and classifies every pair of the ORACLE's list (every
tile of the 3-sigma rectangle: the universe) from first principles:

  must     some in-image pixel (x, y) of the tile has, in float64 from the fp32 conic and in the blend's own formula
           (d = mean - pixel, power = -1/2 (a dx^2 + c dy^2) - b dx dy),  power <= 0  and  power >= -(ln(255 o) + MARGIN).
           MARGIN = 0.005 is half the additive inflation the kernel documents for its tau (+ 0.01) and several hundred times the
           1e-5 relative alpha error of the blend kernels: no pair the blend could accept is excused.  Brute force per pixel.
  may-not  the continuous maximum of `power` over the tile's pixel-centre square [16 t, 16 t + 15]^2 grown by GROW = 0.01 px lies
           below -tau_up, tau_up = (1.01 ln(255 o) + 0.01) (1 + 1e-3): ten times the only slack the kernel's comments claim (1e-4
           relative on tau, 1e-3 px on L / R).  The maximum of a concave quadratic over a square is exact: 0 if the centre lies
           inside, otherwise the best of the four clamped 1-D edge maxima.
  free     everything between: the only slack there is; its share is reported per case.

Where the classes apply (the rules, stated explicitly):
  * o < fp32(1/255): alpha = o exp(power) <= o can never reach 1/255 -- NO tile at all.  must is empty, every pair is may-not.
  * the float64 determinant a c - b^2 of the fp32 conic is not safely positive (<= DET_REL x max(a c, b^2)), or a <= 0, or
    c <= 0: no finite box is claimed -- an infinite box is the FULL rectangle; may-not is empty.
  * may-not "of the box" (cull_variant 1, and cull_variant 2 on rectangles of more than 64 tiles): the tile's grown column or row
    interval misses mean +- h_up, h_up = sqrt(2 tau_up c / det) (x) and sqrt(2 tau_up a / det) (y).
  * may-not "of the ellipse" (cull_variant 2) applies where the kernel claims to cull by the ellipse: on Gaussians whose listed
    rectangle -- the 3-sigma rectangle cut to the box -- has at most 64 tiles.  The reference takes the rectangle of the
    INFLATED box (h_up, grown): it contains the kernel's, so at most 64 tiles there is at most 64 tiles in the kernel.
"""
from __future__ import annotations

import numpy as np

TILE = 16
MARGIN = 0.005
GROW = 0.01
TAU_UP_REL = 1e-3
DET_REL = 1e-5
F32_INV255 = np.float32(1.0) / np.float32(255.0)  # the constant the blend and the kernel compare with
MASK_TILES = 64


def grid(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


# ---------------------------------------------------------------------------------------------------------------- lists
def check_ranges(ranges, N, tag=""):
    """ranges [T, 2] is consistent with a list of N instances: the non-empty tiles' ranges are contiguous in tile order and
    cover [0, N); an empty tile holds (0, 0)."""
    r = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    lo, hi = r[:, 0], r[:, 1]
    assert (hi >= lo).all(), f"{tag}: a range ends before it starts"
    ne = hi > lo
    assert (lo[~ne] == 0).all() and (hi[~ne] == 0).all(), f"{tag}: an empty tile's range is not (0, 0)"
    if N == 0:
        assert not ne.any(), f"{tag}: ranges of an empty list"
        return
    assert ne.any(), f"{tag}: no tile has a range although N = {N}"
    l, h = lo[ne], hi[ne]
    assert l[0] == 0 and h[-1] == N, f"{tag}: ranges cover [{l[0]}, {h[-1]}) instead of [0, {N})"
    assert (l[1:] == h[:-1]).all(), f"{tag}: ranges are not contiguous"


def pair_keys(point_list, ranges, P, tag=""):
    """The list as int64 keys tile * P + gaussian, in list order (ranges are checked first)."""
    pl = np.asarray(point_list).astype(np.int64).reshape(-1)
    check_ranges(ranges, pl.size, tag)
    r = np.asarray(ranges).astype(np.int64).reshape(-1, 2)
    tile = np.repeat(np.arange(r.shape[0], dtype=np.int64), r[:, 1] - r[:, 0])
    assert ((pl >= 0) & (pl < P)).all(), f"{tag}: a Gaussian id outside [0, P)"
    return tile * P + pl


def filter_in_order(universe_keys, keep_keys):
    """Order-preserving filter of the oracle's list by a keep-set (per tile, since the tile is part of the key)."""
    return universe_keys[np.isin(universe_keys, keep_keys)]


def assert_sublist(universe_keys, got_keys, tag=""):
    """got is the universe's list filtered IN ORDER by the set got lists: no reordering (tie order included), no duplicate, no
    foreign pair."""
    want = filter_in_order(universe_keys, got_keys)
    if want.size != got_keys.size or not np.array_equal(want, got_keys):
        foreign = int((~np.isin(got_keys, universe_keys)).sum())
        dup = int(got_keys.size - np.unique(got_keys).size)
        first = int(np.argmax(want[:min(want.size, got_keys.size)] != got_keys[:min(want.size, got_keys.size)])) \
            if min(want.size, got_keys.size) else -1
        raise AssertionError(f"{tag}: list is not an order-preserving sub-list ({got_keys.size} pairs, {foreign} foreign, "
                             f"{dup} duplicates, first difference at position {first})")


def expected_cut_keys(keys, P, depths, zcut):
    """What a list keeps under a per-tile depth cut: the pairs with depths[g] <= zcut[tile], order kept."""
    t, g = keys // P, keys % P
    return keys[~(np.asarray(depths, np.float32)[g] > np.asarray(zcut, np.float32)[t])]


# -------------------------------------------------------------------------------------------------------- classification
def _quad(a, b, c, dx, dy):
    return -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy


def quad_max_over_rect(a, b, c, dxlo, dxhi, dylo, dyhi):
    """Exact maximum of the concave quadratic -1/2 (a dx^2 + c dy^2) - b dx dy (a, c > 0, a c > b^2) over a rectangle."""
    inside = (dxlo <= 0) & (dxhi >= 0) & (dylo <= 0) & (dyhi >= 0)
    best = np.full(np.broadcast(a, dxlo).shape, -np.inf)
    for e in (dxlo, dxhi):
        best = np.maximum(best, _quad(a, b, c, e, np.clip(-b * e / c, dylo, dyhi)))
    for e in (dylo, dyhi):
        best = np.maximum(best, _quad(a, b, c, np.clip(-b * e / a, dxlo, dxhi), e))
    return np.where(inside, 0.0, best)


def gaussian_terms(st):
    """Per-Gaussian float64 quantities of the fp32 state."""
    co = np.asarray(st["conic_opacity"], np.float32)
    a, b, c = (co[:, i].astype(np.float64) for i in range(3))
    o32 = co[:, 3]
    o = o32.astype(np.float64)
    det = a * c - b * b  # (both products are exact in float64: one rounding)
    det_safe = (det > DET_REL * np.maximum(np.abs(a * c), b * b)) & (a > 0) & (c > 0)
    opaque_enough = o32 >= F32_INV255
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.where(opaque_enough, np.log(np.maximum(255.0 * o, 1e-300)), -np.inf)
        tau_nom = 1.01 * ln + 0.01
        tau_up = tau_nom * (1.0 + TAU_UP_REL)
        boxed = det_safe & opaque_enough
        sdet = np.where(boxed, det, 1.0)
        h = {}
        for name, tau in (("nom", tau_nom), ("up", tau_up)):
            t = np.where(boxed, tau, 0.0)
            h[name] = (np.where(boxed, np.sqrt(2.0 * t * c / sdet), np.inf), np.where(boxed, np.sqrt(2.0 * t * a / sdet), np.inf))
    m = np.asarray(st["means2D"], np.float32).astype(np.float64)
    return dict(a=a, b=b, c=c, o=o, o32=o32, det=det, det_safe=det_safe, opaque_enough=opaque_enough, boxed=boxed, ln255o=ln,
                tau_nom=tau_nom, tau_up=tau_up, hx_nom=h["nom"][0], hy_nom=h["nom"][1], hx_up=h["up"][0], hy_up=h["up"][1],
                mx=m[:, 0], my=m[:, 1])


def _box_rect(x0, x1, y0, y1, mx, my, hx, hy, grow):
    """Tile rectangle [bx0, bx1) x [by0, by1): the tiles of [x0, x1) x [y0, y1) whose grown pixel-centre range meets mean +- h."""
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(hx) & np.isfinite(hy)
        hx_, hy_ = np.where(fin, hx, 0.0), np.where(fin, hy, 0.0)
        bx0 = np.maximum(x0, np.ceil((mx - hx_ - grow - (TILE - 1)) / TILE))
        bx1 = np.minimum(x1, np.floor((mx + hx_ + grow) / TILE) + 1)
        by0 = np.maximum(y0, np.ceil((my - hy_ - grow - (TILE - 1)) / TILE))
        by1 = np.minimum(y1, np.floor((my + hy_ + grow) / TILE) + 1)
    bx0, bx1, by0, by1 = (np.where(fin, v, w).astype(np.int64) for v, w in ((bx0, x0), (bx1, x1), (by0, y0), (by1, y1)))
    return bx0, np.maximum(bx1, bx0), by0, np.maximum(by1, by0)


def classify(st, radii, W, H, chunk=1 << 14):
    """-> dict over the oracle's pairs (list order): keys, tile, gid, must, border_only, may_not_box, may_not (cull_variant 2),
    power_max (continuous, grown square; nan where no box is claimed), plus per-Gaussian arrays under "g"."""
    P = int(st["P"])
    gx, gy = grid(W, H)
    keys = pair_keys(st["point_list"], st["ranges"], P, "oracle")
    tile, gid = keys // P, keys % P
    tx, ty = tile % gx, tile // gx
    g = gaussian_terms(st)
    radii = np.asarray(radii).reshape(-1)
    assert (radii[gid] > 0).all()
    # the oracle's rectangle of a Gaussian, read off its list (the list holds every tile of it)
    big = np.iinfo(np.int64).max
    x0 = np.full(P, big); y0 = np.full(P, big); x1 = np.zeros(P, np.int64); y1 = np.zeros(P, np.int64)
    np.minimum.at(x0, gid, tx); np.minimum.at(y0, gid, ty)
    np.maximum.at(x1, gid, tx + 1); np.maximum.at(y1, gid, ty + 1)
    in_list = x1 > 0
    x0[~in_list] = 0; y0[~in_list] = 0
    n_rect = (x1 - x0) * (y1 - y0)
    assert (n_rect == np.asarray(st["tiles_touched"]).astype(np.int64)).all(), "the oracle's lists are not full rectangles"
    g.update(x0=x0, x1=x1, y0=y0, y1=y1, n_rect=n_rect)
    for name in ("nom", "up"):
        bx0, bx1, by0, by1 = _box_rect(x0, x1, y0, y1, g["mx"], g["my"], g["hx_" + name], g["hy_" + name], GROW if name == "up" else 0.0)
        n = (bx1 - bx0) * (by1 - by0)
        n[~g["opaque_enough"]] = 0
        g["box_" + name] = (bx0, bx1, by0, by1)
        g["n_box_" + name] = n
    g["ellipse_claimed"] = g["boxed"] & (g["n_box_up"] <= MASK_TILES)

    # ---- must: brute force over the tile's in-image pixels
    N = keys.size
    must = np.zeros(N, bool)
    border_only = np.zeros(N, bool)
    offs = np.arange(TILE, dtype=np.float64)
    edge = (offs == 0) | (offs == TILE - 1)
    border = edge[:, None] | edge[None, :]
    thr = -(g["ln255o"] + MARGIN)  # (+inf where o < 1/255: nothing qualifies)
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        gi = gid[s:e]
        px = tx[s:e, None] * float(TILE) + offs[None, :]
        py = ty[s:e, None] * float(TILE) + offs[None, :]
        dx = (g["mx"][gi, None] - px)[:, None, :]
        dy = (g["my"][gi, None] - py)[:, :, None]
        power = _quad(g["a"][gi, None, None], g["b"][gi, None, None], g["c"][gi, None, None], dx, dy)
        ok = (power <= 0) & (power >= thr[gi, None, None]) & (px < W)[:, None, :] & (py < H)[:, :, None]
        must[s:e] = ok.any(axis=(1, 2))
        border_only[s:e] = must[s:e] & ~(ok & ~border[None]).any(axis=(1, 2))
    must &= g["opaque_enough"][gid]
    border_only &= must

    # ---- may-not
    lo_x, hi_x = tx * float(TILE) - GROW, tx * float(TILE) + (TILE - 1) + GROW
    lo_y, hi_y = ty * float(TILE) - GROW, ty * float(TILE) + (TILE - 1) + GROW
    mx, my = g["mx"][gid], g["my"][gid]
    boxed = g["boxed"][gid]
    with np.errstate(invalid="ignore"):
        outside_box = boxed & ((lo_x > mx + g["hx_up"][gid]) | (hi_x < mx - g["hx_up"][gid]) |
                               (lo_y > my + g["hy_up"][gid]) | (hi_y < my - g["hy_up"][gid]))
    never = ~g["opaque_enough"][gid]
    may_not_box = outside_box | never
    power_max = np.full(N, np.nan)
    sel = np.nonzero(boxed)[0]
    power_max[sel] = quad_max_over_rect(g["a"][gid[sel]], g["b"][gid[sel]], g["c"][gid[sel]], mx[sel] - hi_x[sel], mx[sel] - lo_x[sel],
                                        my[sel] - hi_y[sel], my[sel] - lo_y[sel])
    with np.errstate(invalid="ignore"):
        outside_ellipse = boxed & (power_max < -g["tau_up"][gid])
    may_not = may_not_box | (outside_ellipse & g["ellipse_claimed"][gid])
    return dict(P=P, W=W, H=H, gx=gx, gy=gy, keys=keys, tile=tile, gid=gid, tx=tx, ty=ty, must=must, border_only=border_only,
                may_not_box=may_not_box, may_not=may_not, outside_ellipse=outside_ellipse, power_max=power_max, g=g)


def free_share(cl):
    """Share of the oracle's pairs that are neither must nor may-not (cull_variant 2): the reference's own slack."""
    n = cl["keys"].size
    return float((~cl["must"] & ~cl["may_not"]).sum()) / n if n else 0.0


# ------------------------------------------------------------------------------------------- checks of the reference itself
def sampled_power_max(cl, idx, n=33):
    """Brute-force dense sampling of the grown tile square (n x n points, corners included) for the pairs idx: the sampled
    maximum and a rigorous bound on how far the true maximum can lie above it (gradient bound x half a cell diagonal)."""
    g, gid = cl["g"], cl["gid"][idx]
    a, b, c = g["a"][gid], g["b"][gid], g["c"][gid]
    span = (TILE - 1) + 2 * GROW
    s = np.linspace(0.0, span, n)
    dx = (g["mx"][gid] - (cl["tx"][idx] * float(TILE) - GROW))[:, None] - s[None, :]
    dy = (g["my"][gid] - (cl["ty"][idx] * float(TILE) - GROW))[:, None] - s[None, :]
    q = _quad(a[:, None, None], b[:, None, None], c[:, None, None], dx[:, None, :], dy[:, :, None])
    smax = q.max(axis=(1, 2))
    # |grad q| = |(a dx + b dy, b dx + c dy)| is convex: its maximum over the square is at a corner
    gmax = np.zeros(len(idx))
    for cx in (dx[:, 0], dx[:, -1]):
        for cy in (dy[:, 0], dy[:, -1]):
            gmax = np.maximum(gmax, np.hypot(a * cx + b * cy, b * cx + c * cy))
    return smax, gmax * (span / (n - 1)) * np.sqrt(0.5)


def float32_accepts(cl, st, idx):
    """Whether a float32 evaluation in the reference's operation order (power = -0.5f (a dx dx + c dy dy) - b dx dy, alpha =
    min(0.99f, o exp(power)), accepted if power <= 0 and alpha >= 1/255) accepts the pair at ANY in-image pixel of its tile."""
    f = np.float32
    co = np.asarray(st["conic_opacity"], np.float32)
    m = np.asarray(st["means2D"], np.float32)
    out = np.zeros(len(idx), bool)
    offs = np.arange(TILE, dtype=np.float32)
    for s in range(0, len(idx), 1 << 14):
        ii = idx[s:s + (1 << 14)]
        gi = cl["gid"][ii]
        px = (cl["tx"][ii, None] * TILE).astype(f) + offs[None, :]
        py = (cl["ty"][ii, None] * TILE).astype(f) + offs[None, :]
        dx = (m[gi, 0, None] - px)[:, None, :]
        dy = (m[gi, 1, None] - py)[:, :, None]
        a, b, c, o = (co[gi, k][:, None, None] for k in range(4))
        power = f(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
        assert power.dtype == np.float32
        with np.errstate(over="ignore", invalid="ignore"):
            alpha = np.minimum(f(0.99), o * np.exp(power))
        ok = (power <= 0) & (alpha >= F32_INV255) & (px < cl["W"])[:, None, :] & (py < cl["H"])[:, :, None]
        out[s:s + (1 << 14)] = ok.any(axis=(1, 2))
    return out
