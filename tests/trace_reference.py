"""Plain numpy reference and result checker of the trace (csrc/render_fwd.hip: render_fwd_k<1, true, false, false>, reached through
goi_raster_trace).  Test infrastructure only; shared by tests/test_trace_reference_cpu.py and tests/test_gpu_trace.py.

THE CONTRACT.  The trace walks every pixel's tile list front to back exactly like the forward blend and, for every contributor whose
alpha exceeds 0.005 (compared in double, as the reference's literal is: cuda_rasterizer/forward.cu:521), adds the pixel's S values
of img_sem to the Gaussian's row of gau_sem [P,S] and S to num_gsem [P].  The reference's own `+=` is not atomic; the product's
contract is the race-free sum, which only a reference of our own can state.

INPUTS are those of tests/blend_reference.py: a Frame (records, lists, ranges and the trace's n_contrib), its Quads, and per
candidate pair (quadrant, list position) the kernel's own fp32 alpha and `hit` = both guard bits of its 64 pixels.  An EVENT of
(pixel, list position pos) happens iff
    the lane is inside the image,  both guards pass,  pos < n_contrib[pixel]  and  float64(alpha_fp32) > 0.005
(`hit and pos < n_contrib` is the kernel's `c`: a pixel still live at pos that passes the guards and T (1 - alpha) >= 1e-4 -- a
hit that fails the last test ends the pixel, so no contributor follows it).  The count is therefore an integer identity for every
Gaussian; the sum is exact up to the order of the fp32 additions.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests.blend_reference import Frame, Quads, U

EVENT_ALPHA = 0.005  # a double literal in the reference and in the kernel


def gamma(k):
    """k u / (1 - k u), u = 2^-24: the relative error bound of k fp32 roundings (Higham, Accuracy and Stability, lemma 3.1)."""
    k = np.asarray(k, np.float64)
    return k * U / (1 - k * U)


@dataclass
class TraceRef:
    count: np.ndarray    # [P] int64 events of each Gaussian
    sum: np.ndarray      # [P,S] float64
    abs_sum: np.ndarray  # [P,S] float64, the same sum over |values|
    stats: dict = field(default_factory=dict)


def events(qd: Quads, alpha, hit, *, threshold=EVENT_ALPHA, strict=True, stop=True, clip=True) -> np.ndarray:
    """[npairs,64] bool: the events.  The keywords state WRONG kernels for the negative controls and are never used by a comparison:
    threshold / strict: another gate (strict False: >=); stop False: hits behind the pixel's n_contrib count too; clip False: a
    lane outside the image scatters every hit above the threshold (such a lane has no n_contrib; its pixel index is 0)."""
    a64 = np.asarray(alpha, np.float32).astype(np.float64)
    big = a64 > threshold if strict else a64 >= threshold
    hit = np.asarray(hit, bool)
    ins = qd.inside[qd.pair_quad]
    live = (qd.pair_pos[:, None] < qd.nc[qd.pair_quad]) if stop else ins
    ev = hit & ins & live & big
    if not clip:
        ev |= hit & ~ins & big
    return ev


def accumulate(fr: Frame, qd: Quads, ev: np.ndarray, img_sem) -> tuple:
    """(count [P] int64, sum [P,S] float64, abs_sum [P,S] float64) of the events `ev`.  The float64 sum of n fp32 values is off by at
    most n 2^-53 of abs_sum, 2^-29 of one fp32 rounding, and exact for integer values below 2^53."""
    img = np.asarray(img_sem)
    S = img.shape[0]
    assert img.shape == (S, fr.H, fr.W) and img.dtype == np.float32, (img.shape, img.dtype)
    i, lane = np.nonzero(ev)
    g = qd.pair_id[i]
    pix = qd.pix[qd.pair_quad[i], lane]
    count = np.bincount(g, minlength=fr.P).astype(np.int64)
    vals = img.reshape(S, -1)[:, pix].astype(np.float64)
    tot, mag = np.zeros((fr.P, S)), np.zeros((fr.P, S))
    for ch in range(S):
        tot[:, ch] = np.bincount(g, weights=vals[ch], minlength=fr.P)
        mag[:, ch] = np.bincount(g, weights=np.abs(vals[ch]), minlength=fr.P)
    return count, tot, mag


def trace_reference(fr: Frame, qd: Quads, alpha, hit, img_sem) -> TraceRef:
    """count, sum, abs_sum and the statistics of one case:
    events; gaussians_with_events; events_at_64_or_later (list positions >= 64: after the first batch the wave stages);
    low_alpha_contributors (contributors with 1/255 <= alpha <= 0.005: they add colour and are not events);
    hits_behind_n_contrib (above the threshold, at or behind the pixel's last contributor: a kernel that goes on scattering after
    the pixel has stopped would count them); lanes_outside (lanes of listed quadrants that lie outside the image) and hits_outside
    (their pairs that pass the guards above the threshold: a kernel that lets them scatter would count them)."""
    hit = np.asarray(hit, bool)
    ev = events(qd, alpha, hit)
    count, tot, mag = accumulate(fr, qd, ev, img_sem)
    ins = qd.inside[qd.pair_quad]
    below = qd.pair_pos[:, None] < qd.nc[qd.pair_quad]
    big = np.asarray(alpha, np.float32).astype(np.float64) > EVENT_ALPHA
    stats = dict(events=int(ev.sum()), gaussians_with_events=int((count > 0).sum()),
                 events_at_64_or_later=int(ev[qd.pair_pos >= 64].sum()),
                 low_alpha_contributors=int((hit & ins & below & ~big).sum()),
                 hits_behind_n_contrib=int((hit & ins & ~below & big).sum()),
                 lanes_outside=int((~qd.inside).sum()), hits_outside=int((hit & ~ins & big).sum()),
                 max_events_of_a_gaussian=int(count.max()) if count.size else 0)
    return TraceRef(count, tot, mag, stats)


def check_trace(ref: TraceRef, gau_sem, num_gsem, S: int, exact: bool) -> dict:
    """num_gsem == S count for EVERY Gaussian; every row of a Gaussian without events is exactly +0; with `exact` (integer-valued
    images whose partial sums all stay below 2^24: every fp32 addition is exact in any order) gau_sem == sum bit for bit; otherwise
    |gau_sem - sum| <= gamma(n - 1) abs_sum, n the Gaussian's events: n - 1 fp32 additions that round (the first lands on the cleared
    +0 exactly), one rounding each, in any order.  Derived; nothing about it is measured.  Returns the largest error in units of
    the bound."""
    got = np.asarray(gau_sem)
    num = np.asarray(num_gsem).astype(np.int64).reshape(-1)
    P = len(ref.count)
    assert got.dtype == np.float32 and got.shape == (P, S) and num.shape == (P,), (got.dtype, got.shape, num.shape)
    want = S * ref.count
    if not np.array_equal(num, want):
        g = int(np.flatnonzero(num != want)[0])
        raise AssertionError(f"num_gsem[{g}] = {num[g]}, must be S x events = {S} x {ref.count[g]} ({int((num != want).sum())} wrong counts)")
    none = ref.count == 0
    if got[none].view(np.uint32).any():
        g = int(np.flatnonzero(none & got.view(np.uint32).any(axis=1))[0])
        raise AssertionError(f"row {g} of gau_sem belongs to a Gaussian without events and is not +0: {got[g]!r}")
    if not np.isfinite(got).all():
        raise AssertionError("gau_sem is not finite")
    if exact:
        assert (ref.abs_sum < 2.0 ** 24).all() and np.array_equal(ref.sum, np.rint(ref.sum)), "the image does not allow the exact check"
        w32 = ref.sum.astype(np.float32)
        if not np.array_equal(got.view(np.uint32), w32.view(np.uint32)):
            g, ch = np.argwhere(got.view(np.uint32) != w32.view(np.uint32))[0]
            raise AssertionError(f"gau_sem[{g},{ch}] = {got[g, ch]!r}, must be exactly {w32[g, ch]!r} ({ref.count[g]} events)")
        return dict(max_ratio=0.0)
    bound = gamma(np.maximum(ref.count - 1, 0))[:, None] * ref.abs_sum
    d = np.abs(got.astype(np.float64) - ref.sum)
    bad = d > bound
    if bad.any():
        g, ch = np.argwhere(bad)[0]
        raise AssertionError(f"gau_sem[{g},{ch}] = {got[g, ch]!r} is {d[g, ch]:.3e} from {ref.sum[g, ch]!r}; bound {bound[g, ch]:.3e} "
                             f"({ref.count[g]} events, sum of magnitudes {ref.abs_sum[g, ch]:.3e}; {int(bad.sum())} elements out)")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, d / bound, 0.0)
    return dict(max_ratio=float(ratio.max()) if ratio.size else 0.0)
