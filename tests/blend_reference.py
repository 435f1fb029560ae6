"""Plain numpy reference and result checkers for the blend kernels (csrc/render_fwd.hip: render_fwd_k; csrc/render_bwd.hip:
render_bwd_rows_k; csrc/render_bwd_sem.hip; csrc/render_bwd_tile.hip) and for the one function pair through which all of them
evaluate a (pixel, Gaussian) pair (csrc/blend_common.h: poly_coefs / eval_poly).  Test infrastructure only.

Shared by tests/test_gpu_blend_rows.py, which feeds it what the device left, and tests/test_blend_reference_cpu.py, which holds
the float64 reference against float64 autograd and feeds every checker deliberately wrong results.

INPUTS are exactly what the kernels read, as the fp32 values they read (class Frame): the records (means2D, conic + opacity,
rgb, depths), the semantic rows, point_list / ranges / n_contrib, out_alpha (T_final = fp32(1 - out_alpha)), bg, the upstream
gradients, and -- per CANDIDATE pair (quadrant, list position), see `candidates` -- E, alpha and the two guard bits of its 64
pixels, either dumped from the device (goi_raster_debug_pair_eval) or evaluated here in the direct form.  With the kernel's own
alphas and last contributors taken as inputs the backward comparison needs no exclusion: every row of every case is compared.

THE BACKWARD of one 8x8 quadrant (render_bwd.hip, header): per pixel, back to front from its last contributor, with
d = <feature, dL/dpixel> + dL/dalpha_out:
    Tn = T / (1 - alpha),  dL/dalpha = (d - R) Tn - T_final / (1 - alpha) <bg, dL/dcolour>,  R <- alpha d + (1 - alpha) R,
    w = alpha Tn,  h = E dL/dalpha  (the 0.99 clamp passed straight through: h carries E, not alpha).
A (quadrant, Gaussian) ROW is  [sum_pix w dL[ch]  for the padded semantic channels, r, g, b, depth |
    -W/2 (a Sx + b Sy), -H/2 (c Sy + b Sx), -1/2 Sxx, -1/2 Sxy, -1/2 Syy, S1 / opacity]
with S_kl = sum_pix h dx^k dy^l, dx = x_gaussian - x_pixel (the reference's conventions, backward.cu: NDC units for the 2D mean,
-1/2 on all three conic elements).  The MAGNITUDE COMPANION of an element is the same sum with every term replaced by its absolute
value: d_abs = sum |f dL| + |dL/dalpha_out|, R_abs by the same recurrence, h_abs = E ((d_abs + R_abs) Tn + |T_final / (1 - alpha)
bg_dot|), and for the moment-derived elements the terms of the expansion around the Gaussian's centre that the kernel evaluates,
sum h_abs (|Dx| + |u|)^k (|Dy| + |v|)^l  (Dx, Dy: centre relative to the quadrant centre; u, v in [-3.5, 3.5]).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

TILE = 16
U = 2.0 ** -24
ALPHA_MIN32 = np.float32(1.0) / np.float32(255.0)
ALPHA_MAX32 = np.float32(0.99)
T_MIN = 1e-4
POWER_TOL = 1e-4
LOG2E = 1.4426950408889634
CLASSES = ("features", "colour_depth", "mean2D", "conic", "opacity")


def nsem_of(S: int) -> int:
    return 4 * ((S + 3) // 4)


def row_floats(S: int) -> int:
    return ((nsem_of(S) + 4 + 6 + 15) // 16) * 16


def sem_row_floats(S: int) -> int:
    return ((nsem_of(S) + 15) // 16) * 16


def element_class(S: int) -> np.ndarray:
    """[nsem + 10] index into CLASSES of every row element."""
    n = nsem_of(S)
    return np.array([0] * n + [1] * 4 + [2] * 2 + [3] * 3 + [4])


# ---- a frame -----------------------------------------------------------------------------------------------------------
@dataclass
class Frame:
    W: int
    H: int
    S: int
    means2D: np.ndarray        # [P,2]
    conic_opacity: np.ndarray  # [P,4] a, b, c, opacity
    rgb: np.ndarray            # [P,3]
    depths: np.ndarray         # [P]
    sem: np.ndarray            # [P,S]
    point_list: np.ndarray     # [N]
    ranges: np.ndarray         # [T,2]
    n_contrib: np.ndarray      # [H*W]
    out_alpha: np.ndarray      # [H*W] fp32
    bg: np.ndarray             # [3]
    extra: dict = field(default_factory=dict)

    @property
    def P(self):
        return self.means2D.shape[0]

    @property
    def N(self):
        return int(self.point_list.shape[0])


@dataclass
class Quads:
    """Geometry of the 4 T quadrants (index 4 tile + q) and their candidate pairs: every (quadrant, list position) of the
    quadrant's tile list, pair index = off[quadrant] + position."""
    gx: int
    gy: int
    Q: int
    px: np.ndarray      # [Q,64] int
    py: np.ndarray
    inside: np.ndarray  # [Q,64] bool
    pix: np.ndarray     # [Q,64] pixel id (0 outside)
    qcx: np.ndarray     # [Q] quadrant centre
    qcy: np.ndarray
    x0: np.ndarray      # [Q] start of the tile's list
    length: np.ndarray  # [Q] its length
    off: np.ndarray     # [Q+1]
    pair_quad: np.ndarray
    pair_pos: np.ndarray
    pair_id: np.ndarray
    nc: np.ndarray      # [Q,64] n_contrib (0 outside)
    qmax: np.ndarray    # [Q] max n_contrib

    @property
    def npairs(self):
        return int(self.off[-1])


def candidates(fr: Frame) -> Quads:
    gx, gy = (fr.W + TILE - 1) // TILE, (fr.H + TILE - 1) // TILE
    Q = gx * gy * 4
    tq = np.arange(Q)
    tile, q = tq >> 2, tq & 3
    qx0 = (tile % gx) * TILE + (q & 1) * 8
    qy0 = (tile // gx) * TILE + (q >> 1) * 8
    lane = np.arange(64)
    px = qx0[:, None] + (lane & 7)[None]
    py = qy0[:, None] + (lane >> 3)[None]
    inside = (px < fr.W) & (py < fr.H)
    pix = np.where(inside, py * fr.W + px, 0)
    r = np.asarray(fr.ranges, dtype=np.int64).reshape(-1, 2)
    x0, length = r[tile, 0], r[tile, 1] - r[tile, 0]
    assert (length >= 0).all() and (r[:, 1] <= fr.N).all(), "ranges point outside the list"
    off = np.zeros(Q + 1, dtype=np.int64)
    off[1:] = np.cumsum(length)
    pair_quad = np.repeat(tq, length)
    pair_pos = np.arange(int(off[-1])) - off[pair_quad]
    pl = np.asarray(fr.point_list, dtype=np.int64)
    pair_id = pl[x0[pair_quad] + pair_pos] if len(pair_quad) else np.zeros(0, np.int64)
    nc = np.where(inside, np.asarray(fr.n_contrib, dtype=np.int64)[pix], 0)
    assert (nc <= length[:, None]).all(), "n_contrib points beyond its tile's list"
    return Quads(gx, gy, Q, px, py, inside, pix, qx0 + 3.5, qy0 + 3.5, x0, length, off, pair_quad, pair_pos, pair_id, nc,
                 nc.max(axis=1))


def requests(qd: Quads) -> np.ndarray:
    """[npairs,2] uint32 (Gaussian id, quadrant index) for goi_raster_debug_pair_eval."""
    return np.stack([qd.pair_id, qd.pair_quad], 1).astype(np.uint32)


# ---- one pair ----------------------------------------------------------------------------------------------------------
def direct_pairs(fr: Frame, qd: Quads, dtype=np.float32, sel=None, alpha_min=None):
    """(E, alpha, below, seen) [n,64] of the candidate pairs `sel` (all), in the reference's direct form evaluated in `dtype`:
    power = -1/2 (a dx^2 + c dy^2) - b dx dy, E = o exp(power), below = power <= kPowerTol."""
    sel = np.arange(qd.npairs) if sel is None else sel
    g, qq = qd.pair_id[sel], qd.pair_quad[sel]
    f = lambda a: np.asarray(a).astype(dtype)  # noqa: E731
    m, co = f(fr.means2D)[g], f(fr.conic_opacity)[g]
    dx = m[:, 0:1] - f(qd.px)[qq]
    dy = m[:, 1:2] - f(qd.py)[qq]
    power = dtype(-0.5) * (co[:, 0:1] * dx * dx + co[:, 2:3] * dy * dy) - co[:, 1:2] * dx * dy
    E = co[:, 3:4] * np.exp(power)
    alpha = np.minimum(dtype(ALPHA_MAX32), E)
    return E.astype(dtype), alpha.astype(dtype), power <= dtype(POWER_TOL), alpha >= dtype(ALPHA_MIN32 if alpha_min is None else alpha_min)


def poly64(fr: Frame, qd: Quads, sel=None):
    """float64 facts about log2 E of the candidate pairs `sel`, from the fp32 record values:
    P64 [n,64] the exact exponent; lim64 [n]; terms_wide [n,64] = |A0| + |u A1| + |v A2| + |A3 u^2| + |A4 u v| + |A5 v^2| with
    exact coefficients; terms_full [n,64] the same with A0, A1, A2 replaced by the sums of the magnitudes of THEIR terms
    (log2 o, a Dx^2, b Dx Dy, c Dy^2; a Dx, b Dy; c Dy, b Dx); S64 [n] the size measure poly_coefs switches on."""
    sel = np.arange(qd.npairs) if sel is None else sel
    g, qq = qd.pair_id[sel], qd.pair_quad[sel]
    m, co = fr.means2D.astype(np.float64)[g], fr.conic_opacity.astype(np.float64)[g]
    a, b, c, o = (co[:, i:i + 1] for i in range(4))
    Dx, Dy = m[:, 0:1] - qd.qcx[qq][:, None], m[:, 1:2] - qd.qcy[qq][:, None]
    u = qd.px[qq] - qd.qcx[qq][:, None]
    v = qd.py[qq] - qd.qcy[qq][:, None]
    with np.errstate(divide="ignore"):
        lo = np.log2(o)
    A0 = lo - 0.5 * LOG2E * (a * Dx * Dx + 2 * b * Dx * Dy + c * Dy * Dy)
    A1, A2 = LOG2E * (a * Dx + b * Dy), LOG2E * (c * Dy + b * Dx)
    A3, A4, A5 = -0.5 * LOG2E * a, -LOG2E * b, -0.5 * LOG2E * c
    P = A0 + u * A1 + v * A2 + A3 * u * u + A4 * u * v + A5 * v * v
    quad = np.abs(A3 * u * u) + np.abs(A4 * u * v) + np.abs(A5 * v * v)
    with np.errstate(invalid="ignore"):
        wide = np.abs(A0) + np.abs(u * A1) + np.abs(v * A2) + quad
        full = (np.abs(lo) + 0.5 * LOG2E * (np.abs(a) * Dx * Dx + 2 * np.abs(b * Dx * Dy) + np.abs(c) * Dy * Dy)
                + LOG2E * np.abs(u) * (np.abs(a * Dx) + np.abs(b * Dy)) + LOG2E * np.abs(v) * (np.abs(c * Dy) + np.abs(b * Dx)) + quad)
    S64 = (np.abs(a) * Dx * Dx + 2 * np.abs(b * Dx * Dy) + np.abs(c) * Dy * Dy)[:, 0]
    return dict(P=P, lim=(lo + POWER_TOL * LOG2E)[:, 0], terms_wide=wide, terms_full=full, S=S64, opacity=o[:, 0])


# Roundings on the path from the record to the exponent (blend_common.h, default build), each at most 2^-24 of a term's magnitude:
#   Dx, Dy = centre - quadrant centre (1 each; they enter A0 twice)                                  4
#   f1 / f2 = fma(a, Dx, b Dy): the product and the fma                                               2
#   A0 = fma(log2e, -1/2 fma(Dx, f1, Dy f2), log2 o): product, two fmas, the constant, v_log_f32 (1 ulp = 2)   6
#   A1, A2 = log2e f: product + constant;  A3, A5, A4: product + constant                             2
#   eval_poly: the packed fma, t1, the inner and the outer fma                                        4
# = 18; the wide path (coefficients formed in fp64 and rounded once) has fewer, and is held to the same count against the
# SMALLER magnitude sum terms_wide.
PAIR_ROUNDINGS = 18
V_EXP_ULP = 2.0 ** -23 * LOG2E * 1.5  # v_exp_f32: 1 ulp of E, as an error of log2 E (+ half an ulp for reading E back)
WIDE_S = 16.0


def check_pairs(fr: Frame, qd: Quads, E, alpha, guards, sel=None, *, check_bound=True) -> dict:
    """The dumped pair evaluation against float64.  E, alpha [n,64] fp32, guards [n,64] uint8 (bit 0 below, bit 1 seen).
    Exact: alpha == min(0.99f, E); seen == (alpha >= fp32(1/255)).  below agrees with float64 outside the band the exponent's
    error bound allows.  |log2 E - P64| <= PAIR_ROUNDINGS 2^-24 terms + the v_exp_f32 ulp, terms = terms_wide for a Gaussian that
    surely takes the fp64 coefficient path (S >= 16 (1 + 2^-20)), terms_full otherwise.  Returns the figures."""
    E, alpha, guards = np.asarray(E, np.float32), np.asarray(alpha, np.float32), np.asarray(guards, np.uint8)
    assert not (guards & 0x80).any(), "a request named no Gaussian or no quadrant"
    if not np.array_equal(alpha.view(np.uint32), np.minimum(ALPHA_MAX32, E).view(np.uint32)):
        i, l = np.argwhere(alpha.view(np.uint32) != np.minimum(ALPHA_MAX32, E).view(np.uint32))[0]
        raise AssertionError(f"pair {i} lane {l}: alpha {alpha[i, l]!r} != min(0.99f, E = {E[i, l]!r})")
    seen = (guards & 2) != 0
    if not np.array_equal(seen, alpha >= ALPHA_MIN32):
        i, l = np.argwhere(seen != (alpha >= ALPHA_MIN32))[0]
        raise AssertionError(f"pair {i} lane {l}: seen bit {seen[i, l]} with alpha {alpha[i, l]!r}")
    p = poly64(fr, qd, sel)
    wide = p["S"] >= WIDE_S * (1 + 2.0 ** -20)
    terms = np.where(wide[:, None], p["terms_wide"], p["terms_full"])
    bound = PAIR_ROUNDINGS * U * terms + V_EXP_ULP
    zero_o = p["opacity"] == 0
    assert not E[zero_o].any() and not seen[zero_o].any(), "a Gaussian of opacity 0 has E != 0"
    below = (guards & 1) != 0
    lim = p["lim"][:, None]
    with np.errstate(invalid="ignore"):
        clear = np.abs(p["P"] - lim) > bound + U * np.abs(lim) * 4
    clear &= ~zero_o[:, None]
    bad = clear & (below != (p["P"] <= lim))
    if bad.any():
        i, l = np.argwhere(bad)[0]
        raise AssertionError(f"pair {i} lane {l}: below bit {below[i, l]} but the exponent is {p['P'][i, l]!r} against {lim[i, 0]!r}")
    ok = (E > 2.0 ** -120) & ~zero_o[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(ok, np.abs(np.log2(E.astype(np.float64)) - p["P"]), 0.0)
        # an E that flushed to zero (or below the normal range) must have a float64 exponent down there too
        assert (p["P"][~ok & ~zero_o[:, None]] < -119).all(), "E is (sub)normal-small where the float64 exponent is not"
        ratio = np.where(ok, err / bound, 0.0)
    out = dict(n=int(E.size), max_err=float(err.max()) if err.size else 0.0, max_ratio=float(ratio.max()) if err.size else 0.0,
               n_wide=int(wide.sum()), max_err_wide=float(err[wide].max()) if wide.any() else 0.0,
               max_terms=float(terms[ok].max()) if ok.any() else 0.0)
    if check_bound and out["max_ratio"] > 1.0:
        i, l = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"pair {i} lane {l}: log2 E = {np.log2(float(E[i, l]))!r} is {err[i, l]:.3e} from the float64 exponent "
                             f"{p['P'][i, l]!r}; bound {bound[i, l]:.3e} (terms {terms[i, l]:.3e}, S {p['S'][i]:.4g})")
    return out


# ---- member masks, qcost, slots ------------------------------------------------------------------------------------------
def member_reference(qd: Quads, hit) -> np.ndarray:
    """[npairs] bool: some pixel of the quadrant has the position below its last contributor and passes both guards."""
    return (np.asarray(hit, bool) & (qd.pair_pos[:, None] < qd.nc[qd.pair_quad])).any(axis=1)


def decode_masks(qd: Quads, qmask0, qmask) -> np.ndarray:
    """[npairs] bool: the member bit of every candidate pair, from the layout documented at member_mask_ptr (common.h): round 0
    of quadrant q of tile t in qmask0[4 t + q]; round r >= 1 of a tile whose list starts at x0 in qmask[4 (x0 / 64 + r) + q]."""
    qmask0, qmask = np.asarray(qmask0, np.uint64), np.asarray(qmask, np.uint64)
    r, j = qd.pair_pos >> 6, (qd.pair_pos & 63).astype(np.uint64)
    tq = qd.pair_quad
    w1 = ((qd.x0[tq] >> 6) + r) * 4 + (tq & 3)
    assert (w1[r > 0] < len(qmask)).all(), "a member word lies outside qmask"
    word = np.where(r == 0, qmask0[tq], qmask[np.minimum(w1, len(qmask) - 1)])
    return ((word >> j) & np.uint64(1)).astype(bool)


def check_masks(qd: Quads, hit, qmask0, qmask, qcost) -> None:
    """qcost[quadrant] == max n_contrib exactly; member bit == member_reference exactly for every position below qcost (bits
    beyond are unspecified)."""
    qcost = np.asarray(qcost, np.int64)
    if not np.array_equal(qcost, qd.qmax):
        q = int(np.flatnonzero(qcost != qd.qmax)[0])
        raise AssertionError(f"qcost[{q}] = {qcost[q]} but the quadrant's largest n_contrib is {qd.qmax[q]}")
    want, got = member_reference(qd, hit), decode_masks(qd, qmask0, qmask)
    look = qd.pair_pos < qd.qmax[qd.pair_quad]
    bad = look & (want != got)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"member bit of quadrant {qd.pair_quad[i]} position {qd.pair_pos[i]} is {got[i]}, must be {want[i]} "
                             f"({int(bad.sum())} wrong bits)")


def slots_reference(fr: Frame, qd: Quads, aux) -> np.ndarray:
    """[npairs] row slot of every candidate pair: (first[g] + rank of the tile among g's listed tiles in tile order) * 4 + q.
    The rank is read off point_list / ranges; first[g] = aux[g][0] is checked to partition [0, N) in steps of the number of tiles
    that list g."""
    aux = np.asarray(aux, np.uint32).reshape(-1, 4)
    r = np.asarray(fr.ranges, np.int64).reshape(-1, 2)
    T = r.shape[0]
    ent_tile = np.repeat(np.arange(T), r[:, 1] - r[:, 0])
    start = np.repeat(r[:, 0], r[:, 1] - r[:, 0])
    ent_index = start + (np.arange(len(ent_tile)) - np.repeat(np.cumsum(r[:, 1] - r[:, 0]) - (r[:, 1] - r[:, 0]), r[:, 1] - r[:, 0]))
    pl = np.asarray(fr.point_list, np.int64)
    assert len(ent_tile) == fr.N and np.array_equal(np.sort(ent_index), np.arange(fr.N)), "ranges do not partition the list"
    g = pl[ent_index]
    o = np.lexsort((ent_tile, g))
    gs = g[o]
    newg = np.r_[True, gs[1:] != gs[:-1]] if len(gs) else np.zeros(0, bool)
    grp_start = np.maximum.accumulate(np.where(newg, np.arange(len(gs)), 0)) if len(gs) else gs
    rank = np.zeros(fr.N, np.int64)
    rank[ent_index[o]] = np.arange(len(gs)) - grp_start
    assert not ((gs[1:] == gs[:-1]) & (ent_tile[o][1:] == ent_tile[o][:-1])).any(), "a Gaussian is listed twice in one tile"
    count = np.bincount(g, minlength=fr.P)
    listed = np.flatnonzero(count)
    first = aux[:, 0].astype(np.int64)
    by_first = listed[np.argsort(first[listed], kind="stable")]
    edges = np.r_[0, np.cumsum(count[by_first])]
    if not (np.array_equal(first[by_first], edges[:-1]) and edges[-1] == fr.N):
        raise AssertionError("the first slots in aux do not partition [0, N) by the Gaussians' tile counts")
    inst = np.zeros(fr.N, np.int64)
    inst[:] = first[pl] + rank
    return inst[qd.x0[qd.pair_quad] + qd.pair_pos] * 4 + (qd.pair_quad & 3)


def check_flags(slots: np.ndarray, member: np.ndarray, flags, N: int) -> None:
    """Validity byte 1 exactly on the slots of member pairs, 0 on every other slot below 4 N."""
    flags = np.asarray(flags, np.uint8)[:4 * N]
    want = np.zeros(4 * N, np.uint8)
    ms = slots[member]
    assert len(np.unique(ms)) == len(ms), "two member pairs share a slot"
    want[ms] = 1
    if not np.array_equal(flags, want):
        s = int(np.flatnonzero(flags != want)[0])
        raise AssertionError(f"validity byte of slot {s} is {flags[s]}, must be {want[s]} ({int((flags != want).sum())} wrong bytes)")


# ---- upstream gradients --------------------------------------------------------------------------------------------------
def upstream_channels(fr: Frame, qd: Quads, up: dict, dtype=np.float64):
    """([Q,64,nsem+4] dL per pixel in the kernels' channel order (sem.., r, g, b, depth), [Q,64] dL/dalpha_out); zero outside the
    image and for absent (None) tensors.  up: color [3,H,W], sem [S,H,W], depth [H,W], alpha [H,W]."""
    n = nsem_of(fr.S)
    dL = np.zeros((qd.Q, 64, n + 4), dtype)
    HW = fr.W * fr.H
    if up.get("sem") is not None:
        dL[:, :, :fr.S] = np.moveaxis(np.asarray(up["sem"]).reshape(fr.S, HW)[:, qd.pix], 0, -1)
    if up.get("color") is not None:
        dL[:, :, n:n + 3] = np.moveaxis(np.asarray(up["color"]).reshape(3, HW)[:, qd.pix], 0, -1)
    if up.get("depth") is not None:
        dL[:, :, n + 3] = np.asarray(up["depth"]).reshape(HW)[qd.pix]
    dLa = np.asarray(up["alpha"]).reshape(HW)[qd.pix].astype(dtype) if up.get("alpha") is not None else np.zeros((qd.Q, 64), dtype)
    dL[~qd.inside] = 0
    dLa = np.where(qd.inside, dLa, 0).astype(dtype)
    return dL, dLa


def features(fr: Frame, dtype=np.float64) -> np.ndarray:
    """[P, nsem+4] staged features in channel order (padded semantics, r, g, b, depth)."""
    n = nsem_of(fr.S)
    f = np.zeros((fr.P, n + 4), dtype)
    f[:, :fr.S] = fr.sem
    f[:, n:n + 3] = fr.rgb
    f[:, n + 3] = fr.depths
    return f


# ---- the backward rows ---------------------------------------------------------------------------------------------------
@dataclass
class Rows:
    rows: np.ndarray           # [npairs, nsem+10]
    mag: np.ndarray | None     # float64 magnitude companions (reference pass only)
    member: np.ndarray         # [npairs] bool
    depth: np.ndarray          # [npairs] contributors walked (back to front, this one included), max over the quadrant's pixels
    npix: np.ndarray           # [npairs] contributing pixels
    dl_max: np.ndarray | None  # [Q, nsem+4] largest |dL| of the channel over the quadrant
    dl_sum: np.ndarray | None  # [Q, nsem+4] sum of |dL|
    wsum: np.ndarray | None    # [npairs] sum of w


def backward_rows(fr: Frame, qd: Quads, up: dict, E, alpha, hit, *, dtype=np.float64, noise=None, direct_moments=False) -> Rows:
    """The rows of every member pair.  dtype float64: the reference, with the magnitude companions.  dtype float32: the YARDSTICK --
    a plain float32 replay of the same formulation (scalar R recurrence, w, h, six quadrant-centred moments accumulated in pixel
    order, expansion around the Gaussian's centre), no split operands, fed the same alphas.
    noise = (rng, eps): every w and h is multiplied by (1 + eps xi), xi = +-1 per (pair, pixel, channel block) -- the error of an
    operand carried with too few bits (tests/test_blend_reference_cpu.py).
    direct_moments (float32 only): sum h dx^k dy^l with dx = x_gaussian - x_pixel formed per pixel, as the reference's backward.cu
    does, instead of the six moments and their expansion -- for context in docs/MEASUREMENT_LOG.md."""
    ref = dtype == np.float64
    n = nsem_of(fr.S)
    nch = n + 4
    dL, dLa = upstream_channels(fr, qd, up, dtype)
    feat = features(fr, dtype)
    bg = np.asarray(fr.bg).astype(dtype)
    bg_dot = bg[0] * dL[:, :, n] + bg[1] * dL[:, :, n + 1] + bg[2] * dL[:, :, n + 2]
    one = dtype(1)
    if "T_final" in fr.extra:  # (frames made here in float64: tests/test_blend_reference_cpu.py)
        T_final = np.where(qd.inside, np.asarray(fr.extra["T_final"])[qd.pix], 0).astype(dtype)
    else:
        T_final = np.where(qd.inside, (np.float32(1) - np.asarray(fr.out_alpha, np.float32))[qd.pix], np.float32(0)).astype(dtype)
    m2 = np.asarray(fr.means2D).astype(dtype)
    co = np.asarray(fr.conic_opacity).astype(dtype)
    lane = np.arange(64)
    u = ((lane & 7) - 3.5).astype(dtype)
    v = ((lane >> 3) - 3.5).astype(dtype)
    perm = np.argsort(-qd.qmax, kind="stable")  # active quadrants are a prefix at every position
    qmax_p = qd.qmax[perm]
    dLp, dLap, bgp, nc_p = dL[perm], dLa[perm], bg_dot[perm], qd.nc[perm]
    absdL = np.abs(dLp) if ref else None
    T, R = T_final[perm].copy(), np.zeros((qd.Q, 64), dtype)
    Tf = T_final[perm]
    Rabs = np.zeros((qd.Q, 64)) if ref else None
    walked = np.zeros((qd.Q, 64), np.int64)
    rows = np.zeros((qd.npairs, nch + 6), dtype)
    mag = np.zeros((qd.npairs, nch + 6)) if ref else None
    wsum = np.zeros(qd.npairs) if ref else None
    member = np.zeros(qd.npairs, bool)
    depth = np.zeros(qd.npairs, np.int64)
    npix = np.zeros(qd.npairs, np.int64)
    E, alpha, hit = np.asarray(E), np.asarray(alpha), np.asarray(hit, bool)
    half_W, half_H = dtype(0.5 * fr.W), dtype(0.5 * fr.H)
    for pos in range(int(qmax_p[0]) - 1 if qd.Q else -1, -1, -1):
        k = int(np.searchsorted(-qmax_p, -pos, side="left"))  # quadrants with qmax > pos
        idx = qd.off[perm[:k]] + pos
        c = hit[idx] & (pos < nc_p[:k])
        any_c = c.any(axis=1)
        if not any_c.any():
            continue
        g = qd.pair_id[idx]
        a_, E_ = alpha[idx].astype(dtype), E[idx].astype(dtype)
        f = feat[g]
        dot = np.matmul(dLp[:k], f[:, :, None])[:, :, 0] + dLap[:k]
        one_m_a = one - a_
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            Tn = T[:k] / one_m_a
            dLdo = (dot - R[:k]) * Tn - (Tf[:k] / one_m_a) * bgp[:k]
            w = np.where(c, a_ * Tn, 0).astype(dtype)
            h = np.where(c, E_ * dLdo, 0).astype(dtype)
            if ref:
                dabs = np.matmul(absdL[:k], np.abs(f)[:, :, None])[:, :, 0] + np.abs(dLap[:k])
                habs = np.where(c, E_ * ((dabs + Rabs[:k]) * Tn + np.abs((Tf[:k] / one_m_a) * bgp[:k])), 0.0)
                Rabs[:k] = np.where(c, a_ * dabs + one_m_a * Rabs[:k], Rabs[:k])
            R[:k] = np.where(c, a_ * dot + one_m_a * R[:k], R[:k])
            T[:k] = np.where(c, Tn, T[:k])
        walked[:k] += c
        if noise is not None:
            rng, eps = noise
            w = (w * (1 + eps * rng.choice([-1.0, 1.0], size=w.shape))).astype(dtype)
            h = (h * (1 + eps * rng.choice([-1.0, 1.0], size=h.shape))).astype(dtype)
        Dx = (m2[g, 0] - qd.qcx[perm[:k]].astype(dtype))[:, None]
        Dy = (m2[g, 1] - qd.qcy[perm[:k]].astype(dtype))[:, None]
        ca, cb, cc, op = co[g, 0], co[g, 1], co[g, 2], co[g, 3]
        out = np.zeros((k, nch + 6), dtype)
        if ref:
            out[:, :nch] = np.matmul(w[:, None, :], dLp[:k])[:, 0]
            dx, dy = Dx - u[None], Dy - v[None]
            m0, sx, sy = h.sum(1), (h * dx).sum(1), (h * dy).sum(1)
            sxx, sxy, syy = (h * dx * dx).sum(1), (h * dx * dy).sum(1), (h * dy * dy).sum(1)
            ax, ay = np.abs(Dx) + np.abs(u)[None], np.abs(Dy) + np.abs(v)[None]
            M = np.zeros((k, nch + 6))
            M[:, :nch] = np.matmul(w[:, None, :], absdL[:k])[:, 0]
            SX, SY = (habs * ax).sum(1), (habs * ay).sum(1)
            M[:, nch + 0] = half_W * (np.abs(ca) * SX + np.abs(cb) * SY)
            M[:, nch + 1] = half_H * (np.abs(cc) * SY + np.abs(cb) * SX)
            M[:, nch + 2] = 0.5 * (habs * ax * ax).sum(1)
            M[:, nch + 3] = 0.5 * (habs * ax * ay).sum(1)
            M[:, nch + 4] = 0.5 * (habs * ay * ay).sum(1)
            with np.errstate(divide="ignore", invalid="ignore"):
                M[:, nch + 5] = habs.sum(1) / op
            mag[idx[any_c]] = M[any_c]
            wsum[idx[any_c]] = w.sum(1)[any_c]
        else:
            seq = lambda x: np.cumsum(x, axis=1, dtype=dtype)[:, -1]  # noqa: E731  (cumsum adds strictly in order)
            out[:, :nch] = seq(w[:, :, None] * dLp[:k])
            b0, bu, bv = seq(h), seq(h * u[None]), seq(h * v[None])
            buu, buv, bvv = seq(h * (u * u)[None]), seq(h * (u * v)[None]), seq(h * (v * v)[None])
            two = dtype(2)
            m0 = b0
            if direct_moments:
                pq = perm[:k]
                dx = m2[g, 0][:, None] - qd.px[pq].astype(dtype)
                dy = m2[g, 1][:, None] - qd.py[pq].astype(dtype)
                sx, sy = seq(h * dx), seq(h * dy)
                sxx, sxy, syy = seq(h * dx * dx), seq(h * dx * dy), seq(h * dy * dy)
            else:
                Dx, Dy = Dx[:, 0], Dy[:, 0]
                sx, sy = Dx * b0 - bu, Dy * b0 - bv
                sxx = Dx * Dx * b0 - two * Dx * bu + buu
                sxy = Dx * Dy * b0 - Dx * bv - Dy * bu + buv
                syy = Dy * Dy * b0 - two * Dy * bv + bvv
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, nch + 0] = -half_W * (ca * sx + cb * sy)
            out[:, nch + 1] = -half_H * (cc * sy + cb * sx)
            out[:, nch + 2] = dtype(-0.5) * sxx
            out[:, nch + 3] = dtype(-0.5) * sxy
            out[:, nch + 4] = dtype(-0.5) * syy
            out[:, nch + 5] = m0 / op
        sel = idx[any_c]
        rows[sel] = out[any_c]
        member[sel] = True
        depth[sel] = np.where(c, walked[:k], 0).max(axis=1)[any_c]
        npix[sel] = c.sum(axis=1)[any_c]
    dl_max = np.abs(dL).max(axis=1) if ref else None
    dl_sum = np.abs(dL).sum(axis=1) if ref else None
    return Rows(rows, mag, member, depth, npix, dl_max, dl_sum, wsum)


def per_gaussian_sums(fr: Frame, qd: Quads, rw: Rows) -> np.ndarray:
    """[P, nsem+10] float64: every Gaussian's rows added up."""
    out = np.zeros((fr.P, rw.rows.shape[1]))
    np.add.at(out, qd.pair_id[rw.member], rw.rows[rw.member].astype(np.float64))
    return out


# ---- tolerances ----------------------------------------------------------------------------------------------------------
# Roundings that form ONE term of a row element, besides the 3 per walked contributor of the T (v_rcp_f32: 1 ulp = 2, the product 1)
# and R chains: the <feature, dL> dot (two chains of 1 + nsem / 4 packed FMAs and two adds: counted as nsem / 2 + 4), dotv - R,
# the two products and the difference of dL/dalpha, T_final inv, E dL/dalpha (6), alpha Tn (1), the f16 / bf16 operand splits
# (2^-22 per weight and per dL: 8) and the expansion around the centre with the final scaling (8).
def n_terms(S: int) -> int:
    return 64 + nsem_of(S) // 2 + 4 + 6 + 1 + 8 + 8


def hard_ceiling(S: int, rw: Rows) -> np.ndarray:
    """[npairs, nsem+10]: (n_terms + 3 depth) 2^-24 M, the any-order summation bound of 64 pixel terms that each carry the
    roundings counted above."""
    return (n_terms(S) + 3 * rw.depth)[:, None] * U * rw.mag


def feature_term(S: int, qd: Quads, rw: Rows) -> np.ndarray:
    """[npairs, nsem+10]: what the split-f16 B operand (blend_common.h: f16_b_operand) may lose of dL besides the 2^-22 per
    product counted in n_terms: a value more than 2^17 below its channel's largest |dL| of the quadrant keeps 2^-25 of THAT
    (scaled to 2^15 the lo plane's last bit is 2^-10: 2^-25 of the top, taken twice for the rounding of hi and lo), times the
    weights it meets -- 2^-24 max|dL_ch| sum w; and the unscaling of the weights' own floor 2^-25 / 2^15: 2^-40 sum |dL|.  Zero for
    the moment-derived elements."""
    nch = nsem_of(S) + 4
    out = np.zeros_like(rw.mag)
    out[:, :nch] = U * rw.dl_max[qd.pair_quad] * rw.wsum[:, None] + 2.0 ** -40 * rw.dl_sum[qd.pair_quad]
    return out


def normalised_errors(S: int, rw: Rows, got: np.ndarray, extra: np.ndarray | None = None):
    """(err [m, nsem+10] = max(0, |got - reference| - extra) / M over the member pairs (0 where M == 0), exact_zero_ok: every
    element whose companion is 0 is exactly 0)."""
    mem = rw.member
    ref, M = rw.rows[mem], rw.mag[mem]
    d = np.abs(np.asarray(got, np.float64)[mem] - ref)
    if extra is not None:
        d = np.maximum(0.0, d - extra[mem])
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(M > 0, d / M, 0.0)
    zero_ok = bool((np.asarray(got)[mem][M == 0] == 0).all())
    return e, zero_ok


def class_stats(S: int, err: np.ndarray) -> dict:
    """{class: (median, p99, max, n)} of the normalised errors, padded semantic channels left out."""
    cls = element_class(S)
    keep = np.ones(len(cls), bool)
    keep[S:nsem_of(S)] = False
    out = {}
    for ci, name in enumerate(CLASSES):
        e = err[:, (cls == ci) & keep].reshape(-1)
        out[name] = (float(np.median(e)), float(np.quantile(e, 0.99)), float(e.max()), int(e.size)) if e.size else (0.0, 0.0, 0.0, 0)
    return out


def pooled_stats(S_list, err_list) -> dict:
    cls_err = {name: [] for name in CLASSES}
    for S, err in zip(S_list, err_list):
        cls = element_class(S)
        keep = np.ones(len(cls), bool)
        keep[S:nsem_of(S)] = False
        for ci, name in enumerate(CLASSES):
            cls_err[name].append(err[:, (cls == ci) & keep].reshape(-1))
    out = {}
    for name, parts in cls_err.items():
        e = np.concatenate(parts) if parts else np.zeros(0)
        out[name] = (float(np.median(e)), float(np.quantile(e, 0.99)), float(e.max()), int(e.size)) if e.size else (0.0, 0.0, 0.0, 0)
    return out


# The YARDSTICK's normalised error |x - f64| / M per element class -- (median, 99th percentile, maximum), pooled over the 47 runs of
# tests/blend_cases.py::all_runs() and the 32 frames of tests/channel_count_cases.py -- measured on the CPU with
# tools/blend_yardstick.py --all (float32 direct-form alphas standing in for the device's): docs/MEASUREMENT_LOG.md, "Direct test of
# the blend kernels" and "Every semantic width 1..32 through the frame kernels" (the figures over the 47 runs alone, which stood
# here before the 32 frames existed, are kept there; the three maxima did not move, so no element's tolerance did).  The gate is
# 4 x the first two and 16 x the third (check_gate, element_tolerance): the 4 x covers the 2^-22 per product of the split operands
# against fp32's 2^-24.
GATE = {
    "features": (0.451 * U, 3.825 * U, 39.316 * U),
    "colour_depth": (0.442 * U, 3.682 * U, 36.859 * U),
    "mean2D": (0.044 * U, 0.544 * U, 4.899 * U),
    "conic": (0.054 * U, 0.569 * U, 4.832 * U),
    "opacity": (0.094 * U, 1.155 * U, 7.054 * U),
}


def check_gate(stats: dict, gate: dict, what: str = "") -> None:
    """The measured gate: per class, median and 99th percentile of the normalised error within 4 x the yardstick's, the maximum
    within 16 x its maximum.  gate: {class: (median, p99, max)} of the YARDSTICK."""
    for name in CLASSES:
        med, p99, mx, n = stats[name]
        if n == 0:
            continue
        gm, gp, gx = gate[name][:3]
        assert med <= 4 * gm, f"{what}{name}: median normalised error {med / U:.3f} x 2^-24 > 4 x the yardstick's {gm / U:.3f}"
        assert p99 <= 4 * gp, f"{what}{name}: p99 normalised error {p99 / U:.3f} x 2^-24 > 4 x the yardstick's {gp / U:.3f}"
        assert mx <= 16 * gx, f"{what}{name}: max normalised error {mx / U:.3f} x 2^-24 > 16 x the yardstick's {gx / U:.3f}"


def element_tolerance(S: int, qd: Quads, rw: Rows, gate: dict, *, split: bool = True) -> np.ndarray:
    """[npairs, nsem+10]: what ONE element may be off: the derived feature term plus 16 x the yardstick's maximum of its class
    times its companion, and never more than the hard ceiling (plus the derived term)."""
    cls = element_class(S)
    gmax = np.array([16 * gate[CLASSES[c]][2] for c in cls])
    ft = feature_term(S, qd, rw) if split else np.zeros_like(rw.mag)
    return ft + np.minimum(gmax[None] * rw.mag, hard_ceiling(S, rw))


def check_rows(S: int, qd: Quads, rw: Rows, got: np.ndarray, gate: dict, what: str = "", *, split: bool = True) -> np.ndarray:
    """Every element of every member row: finite, padded semantic channels exactly 0, an element whose companion is 0 exactly 0,
    every other within element_tolerance.  Returns the normalised errors (after the derived feature term) for the pooled gate."""
    got = np.asarray(got)
    mem = rw.member
    g = got[mem].astype(np.float64)
    if not np.isfinite(g).all():
        i, e = np.argwhere(~np.isfinite(g))[0]
        raise AssertionError(f"{what}: element {e} of member pair {np.flatnonzero(mem)[i]} was not written (or is not finite)")
    n = nsem_of(S)
    if got[mem][:, S:n].any():
        raise AssertionError(f"{what}: a padded semantic channel is not exactly 0")
    tol = element_tolerance(S, qd, rw, gate, split=split)[mem]
    d = np.abs(g - rw.rows[mem])
    bad = d > tol
    if bad.any():
        i, e = np.argwhere(bad)[np.argmax((d / np.maximum(tol, 1e-300))[bad])]
        p = int(np.flatnonzero(mem)[i])
        raise AssertionError(f"{what}: pair {p} (quadrant {qd.pair_quad[p]}, position {qd.pair_pos[p]}, Gaussian {qd.pair_id[p]}) "
                             f"element {e}: {g[i, e]!r} is {d[i, e]:.3e} from {rw.rows[mem][i, e]!r}, tolerance {tol[i, e]:.3e} "
                             f"(companion {rw.mag[mem][i, e]:.3e}, depth {rw.depth[p]}; {int(bad.sum())} elements out)")
    err, zero_ok = normalised_errors(S, rw, got, feature_term(S, qd, rw) if split else None)
    assert zero_ok, f"{what}: an element whose every term is 0 is not exactly 0"
    return err


# ---- the forward ---------------------------------------------------------------------------------------------------------
def forward_reference(fr: Frame, qd: Quads, alpha, hit) -> dict:
    """float64 composite of every pixel from the kernel's own alphas, guard bits and last contributors:
    maps [nsem+4, Q, 64] (+ T bg for r, g, b -> `color`), their magnitude companions, T after the last contributor, the pixel's
    depth k (contributors), and the product T (1 - alpha) at its STOPPER (the first hit at or behind n_contrib; NaN: none)."""
    n = nsem_of(fr.S)
    feat = features(fr)
    perm = np.argsort(-qd.length, kind="stable")
    len_p, nc_p = qd.length[perm], qd.nc[perm]
    T = np.ones((qd.Q, 64))
    acc = np.zeros((qd.Q, 64, n + 4))
    mag = np.zeros((qd.Q, 64, n + 4))
    k_depth = np.zeros((qd.Q, 64), np.int64)
    stop = np.full((qd.Q, 64), np.nan)
    last_hit = np.zeros((qd.Q, 64), bool)
    alpha, hit = np.asarray(alpha), np.asarray(hit, bool)
    for pos in range(int(len_p[0]) if qd.Q else 0):
        k = int(np.searchsorted(-len_p, -pos, side="left"))
        idx = qd.off[perm[:k]] + pos
        a_ = alpha[idx].astype(np.float64)
        h_ = hit[idx] & qd.inside[perm[:k]]
        c = h_ & (pos < nc_p[:k])
        w = np.where(c, a_ * T[:k], 0.0)
        f = feat[qd.pair_id[idx]]
        acc[:k] += w[:, :, None] * f[:, None, :]
        mag[:k] += w[:, :, None] * np.abs(f)[:, None, :]
        first_after = h_ & (pos >= nc_p[:k]) & np.isnan(stop[:k])
        stop[:k] = np.where(first_after, T[:k] * (1 - a_), stop[:k])
        T[:k] = np.where(c, T[:k] * (1 - a_), T[:k])
        k_depth[:k] += c
        last_hit[:k] |= h_ & (pos == nc_p[:k] - 1)
    inv = np.argsort(perm)
    return dict(acc=acc[inv], mag=mag[inv], T=T[inv], k=k_depth[inv], stop=stop[inv], last_hit=last_hit[inv])


def check_forward(fr: Frame, qd: Quads, fw: dict, maps: dict, gate: dict, *, colour_only: bool = False) -> dict:
    """n_contrib against the stop rule in float64 -- the last contributor is a hit, the product after it is not below 1e-4, the
    stopper's product is below it, each within (k + 2) 2^-23 relative (k: the pixel's contributors; two roundings per factor of
    the fp32 product chain) -- and out_alpha and the four maps against the float64 composite within the element's magnitude
    companion times the gate (16 x the yardstick's maximum: features for the semantic map, colour / depth for the others).
    maps: color [3,HW], sem [S,HW], depth [HW], alpha [HW], all four -- or, with colour_only (a trace has no other map), `color`
    alone.  Returns the largest normalised errors."""
    want_keys = {"color"} if colour_only else {"color", "sem", "depth", "alpha"}
    assert set(maps) == want_keys, f"maps must hold exactly {sorted(want_keys)}, got {sorted(maps)}"
    ins = qd.inside
    nc = qd.nc
    assert (fw["last_hit"] | (nc == 0))[ins].all(), "a pixel's last contributor is not a pair that passes the guards"
    slack = (fw["k"] + 2) * 2.0 ** -23
    low = ins & (nc > 0) & (fw["T"] < T_MIN * (1 - slack))
    assert not low.any(), f"{int(low.sum())} pixels kept a contributor that brings the product below 1e-4"
    with np.errstate(invalid="ignore"):
        high = ins & (fw["stop"] >= T_MIN * (1 + slack))
    assert not high.any(), f"{int(high.sum())} pixels stopped at a Gaussian whose product is not below 1e-4"
    n = nsem_of(fr.S)
    bg = np.asarray(fr.bg, np.float64)
    pix = qd.pix[ins]
    out = {}

    def cmp(name, got, want, M, g):
        d = np.abs(np.asarray(got, np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(M > 0, d / M, np.where(d == 0, 0.0, np.inf))
        out[name] = float(e.max()) if e.size else 0.0
        assert out[name] <= g, f"{name}: normalised error {out[name] / U:.2f} x 2^-24 beyond the gate {g / U:.2f} x 2^-24"

    gf, gc = 16 * gate["features"][2], 16 * gate["colour_depth"][2]
    acc, mag, T = fw["acc"][ins], fw["mag"][ins], fw["T"][ins]
    for ch in range(0 if colour_only else fr.S):
        cmp("sem", np.asarray(maps["sem"]).reshape(fr.S, -1)[ch, pix], acc[:, ch], mag[:, ch], gf)
    for ch in range(3):
        cmp("color", np.asarray(maps["color"]).reshape(3, -1)[ch, pix], acc[:, n + ch] + T * bg[ch], mag[:, n + ch] + T * abs(bg[ch]), gc)
    if not colour_only:
        cmp("depth", np.asarray(maps["depth"]).reshape(-1)[pix], acc[:, n + 3], mag[:, n + 3], gc)
    if not colour_only:
        cmp("alpha", np.asarray(maps["alpha"]).reshape(-1)[pix], 1 - T, np.ones_like(T), gc)
    return out


# ---- frames without a device -------------------------------------------------------------------------------------------------
def cpu_frame(W, H, means2D, conic_opacity, rgb, depths, sem, bg, *, radius=None, rects=None, dtype=np.float32,
              alpha_min=None) -> tuple:
    """A frame whose lists, last contributors and out_alpha are made here: every Gaussian is listed in the tiles of its rectangle
    (rects, or radius pixels around the centre; neither: every tile), lists in depth order (ties by id), pairs evaluated in the direct form in
    `dtype`, the forward's stop rule applied in `dtype`.  Returns (Frame, Quads, E, alpha, hit)."""
    P = len(depths)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    order = np.lexsort((np.arange(P), np.asarray(depths, np.float32)))
    lists = []
    m = np.asarray(means2D, np.float64)
    for t in range(gx * gy):
        tx, ty = t % gx, t // gx
        if rects is not None:  # [P,4] tile rectangle x0, y0, x1, y1 (exclusive upper corner)
            ok = (rects[:, 0] <= tx) & (tx < rects[:, 2]) & (rects[:, 1] <= ty) & (ty < rects[:, 3])
        elif radius is None:
            ok = np.ones(P, bool)
        else:
            r = np.broadcast_to(np.asarray(radius, np.float64), (P,))
            ok = ((m[:, 0] + r >= tx * TILE) & (m[:, 0] - r <= tx * TILE + 15) & (m[:, 1] + r >= ty * TILE)
                  & (m[:, 1] - r <= ty * TILE + 15))
        lists.append(order[ok[order]])
    lens = np.array([len(x) for x in lists])
    ranges = np.stack([np.cumsum(lens) - lens, np.cumsum(lens)], 1).astype(np.uint32)
    keep = np.float32 if dtype == np.float32 else np.float64
    fr = Frame(W, H, sem.shape[1], np.asarray(means2D, keep), np.asarray(conic_opacity, keep),
               np.asarray(rgb, keep), np.asarray(depths, keep), np.asarray(sem, keep),
               np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, np.uint32), ranges,
               np.zeros(W * H, np.uint32), np.zeros(W * H, np.float32), np.asarray(bg, keep))
    qd = candidates(fr)
    E, alpha, below, seen = direct_pairs(fr, qd, dtype, alpha_min=alpha_min)  # (alpha_min: the kernels' fp32(1/255) unless given)
    hit = below & seen
    perm = np.argsort(-qd.length, kind="stable")
    len_p = qd.length[perm]
    T = np.where(qd.inside[perm], dtype(1), dtype(0)).astype(dtype)
    Tout = np.ones((qd.Q, 64), dtype)
    nc = np.zeros((qd.Q, 64), np.int64)
    for pos in range(int(len_p[0]) if qd.Q else 0):
        k = int(np.searchsorted(-len_p, -pos, side="left"))
        idx = qd.off[perm[:k]] + pos
        test_T = (T[:k] * (dtype(1) - alpha[idx])).astype(dtype)
        c0 = hit[idx] & (T[:k] != 0)
        ok = test_T >= dtype(T_MIN)
        c = c0 & ok
        Tout[:k] = np.where(c, test_T, Tout[:k])
        nc[:k] = np.where(c, pos + 1, nc[:k])
        T[:k] = np.where(c0, np.where(ok, test_T, dtype(0)), T[:k])
    inv = np.argsort(perm)
    nc, Tout = nc[inv], Tout[inv]
    fr.n_contrib[qd.pix[qd.inside]] = nc[qd.inside]
    fr.out_alpha[qd.pix[qd.inside]] = (np.float32(1) - Tout.astype(np.float32))[qd.inside]
    if dtype == np.float64:
        tf = np.zeros(W * H)
        tf[qd.pix[qd.inside]] = Tout[qd.inside]
        fr.extra["T_final"] = tf
    qd = candidates(fr)
    return fr, qd, E, alpha, hit
