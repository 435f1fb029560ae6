"""numpy replay of csrc/contrib.hip (goi_raster_contrib_frame) on the candidate pairs of tests/blend_reference.py, and a plain
per-pixel Python loop of the same rule.  Test infrastructure only.

The rule, per pixel inside the image, over its tile's list front to back, with T = 1 at the start: a candidate whose two guard
bits are set (`hit`) on a pixel that is still live has  w = alpha * T  and  test_T = T * (1 - alpha)  (one rounding per
operation, in `dtype`).  test_T >= 1e-4: the candidate CONTRIBUTES, T <- test_T.  Otherwise it is the pixel's STOPPER and the
pixel is finished.  peak[g] = max of w over g's contributions and stops; top_id / top_w = the pixel's contributor of largest w,
the front-most of equals (strict >), -1 / 0 where nothing contributed.
"""
from __future__ import annotations

import numpy as np

from tests import blend_reference as BR


def replay(fr: BR.Frame, qd: BR.Quads, alpha, hit, dtype=np.float32):
    """alpha, hit: [npairs,64] per candidate pair (quadrant, list position) and lane, as goi_raster_debug_pair_eval dumps them
    (hit = both guard bits).  -> (peak [P], top_id [H*W] int32, top_w [H*W]) in `dtype`, every position of a round evaluated
    for all quadrants at once."""
    alpha, hit = np.asarray(alpha).astype(dtype), np.asarray(hit, bool)
    one, tmin = dtype(1), dtype(BR.T_MIN)
    perm = np.argsort(-qd.length, kind="stable")
    len_p = qd.length[perm]
    T = np.where(qd.inside[perm], one, dtype(0)).astype(dtype)
    best_w = np.zeros((qd.Q, 64), dtype)
    best_id = np.full((qd.Q, 64), -1, np.int32)
    peak = np.zeros(fr.P, dtype)
    for pos in range(int(len_p[0]) if qd.Q else 0):
        k = int(np.searchsorted(-len_p, -pos, side="left"))
        idx = qd.off[perm[:k]] + pos
        a = alpha[idx]
        live_hit = hit[idx] & (T[:k] != 0)
        w = np.where(live_hit, (a * T[:k]).astype(dtype), dtype(0))
        test_T = (T[:k] * (one - a).astype(dtype)).astype(dtype)
        ok = test_T >= tmin
        np.maximum.at(peak, qd.pair_id[idx], w.max(axis=1))
        better = live_hit & ok & (w > best_w[:k])
        best_w[:k] = np.where(better, w, best_w[:k])
        best_id[:k] = np.where(better, qd.pair_id[idx][:, None].astype(np.int32), best_id[:k])
        T[:k] = np.where(live_hit, np.where(ok, test_T, dtype(0)), T[:k])
    inv = np.argsort(perm)
    best_w, best_id = best_w[inv], best_id[inv]
    top_id = np.full(fr.W * fr.H, -1, np.int32)
    top_w = np.zeros(fr.W * fr.H, dtype)
    top_id[qd.pix[qd.inside]] = best_id[qd.inside]
    top_w[qd.pix[qd.inside]] = best_w[qd.inside]
    return peak, top_id, top_w


def pixel_loop(fr: BR.Frame, qd: BR.Quads, alpha, hit):
    """The same rule as one plain float64 loop per pixel.  -> (peak [P], top_id [H*W], top_w [H*W], events): events is a list of
    (pixel, Gaussian, w, test_T, contributed) for every pair that passed the guards on a live pixel."""
    peak = np.zeros(fr.P)
    top_id = np.full(fr.W * fr.H, -1, np.int32)
    top_w = np.zeros(fr.W * fr.H)
    events = []
    for q in range(qd.Q):
        for lane in range(64):
            if not qd.inside[q, lane]:
                continue
            pix = int(qd.pix[q, lane])
            T, bw, bi = 1.0, 0.0, -1
            for pos in range(int(qd.length[q])):
                i = int(qd.off[q]) + pos
                if not hit[i, lane]:
                    continue
                g, a = int(qd.pair_id[i]), float(alpha[i, lane])
                w = a * T
                test_T = T * (1.0 - a)
                peak[g] = max(peak[g], w)
                contributed = test_T >= BR.T_MIN
                events.append((pix, g, w, test_T, contributed))
                if not contributed:
                    break
                if w > bw:
                    bw, bi = w, g
                T = test_T
            top_id[pix], top_w[pix] = bi, bw
    return peak, top_id, top_w, events
