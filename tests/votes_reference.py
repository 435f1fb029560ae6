"""numpy replay of csrc/contrib.hip's votes (goi_raster_contrib_votes) on the candidate pairs of tests/blend_reference.py, a plain
loop over the events of contrib_reference.pixel_loop, and the label maps both test files use.  Test infrastructure only.

The rule: contrib_reference's walk; every candidate that CONTRIBUTES to a live pixel inside the image (guards passed and
test_T >= 1e-4 -- the stopper is excluded) whose label l = labels[pixel] is in [0, K) adds  q = rint(w * 2^24)  (half to even,
the product exact) to votes[Gaussian, l], summed as int64.
"""
from __future__ import annotations

import numpy as np

from tests import blend_reference as BR

UNIT = 2 ** 24
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
MAP_KINDS = ("uniform", "half-plane", "checkerboard", "64-distinct")


def label_map(kind: str, W: int, H: int, ignored: bool = False, seed: int = 0):
    """-> (labels int32 [H*W], K).  uniform: all 0, K = 1; half-plane: 1 right of a slanted line that is aligned to no multiple
    of 8, K = 2; checkerboard: 1-pixel squares, K = 2; 64-distinct: (x % 8) + 8 (y % 8), K = 64.  ignored: a pseudo-random tenth
    of the pixels takes one of -1, K, INT_MAX, INT_MIN."""
    y, x = np.mgrid[0:H, 0:W]
    if kind == "uniform":
        lab, K = np.zeros((H, W), np.int64), 1
    elif kind == "half-plane":
        lab, K = (3 * x + y > 3 * (W // 2) + 5).astype(np.int64), 2
    elif kind == "checkerboard":
        lab, K = (x + y) & 1, 2
    elif kind == "64-distinct":
        lab, K = (x % 8) + 8 * (y % 8), 64
    else:
        raise KeyError(kind)
    lab = lab.reshape(-1).astype(np.int64)
    if ignored:
        rng = np.random.default_rng(seed + 17 * MAP_KINDS.index(kind))
        drop = rng.random(W * H) < 0.1
        lab = np.where(drop, rng.choice(np.array([-1, K, INT_MAX, INT_MIN]), W * H), lab)
    return lab.astype(np.int32), K


def quad_labels(qd: BR.Quads, labels, K: int) -> np.ndarray:
    """[Q,64] the label of each lane's pixel, -1 where the pixel is outside the image or its label outside [0, K)"""
    lab = np.asarray(labels, np.int64).reshape(-1)[qd.pix]
    return np.where(qd.inside & (lab >= 0) & (lab < K), lab, -1)


def contributions(fr: BR.Frame, qd: BR.Quads, alpha, hit, dtype=np.float32):
    """alpha, hit: [npairs,64] as for contrib_reference.replay.  -> (pixel, Gaussian, q), three int64 arrays with one entry per
    pair that contributes to a live pixel inside the image, every position of a round evaluated for all quadrants at once,
    the arithmetic in `dtype`."""
    alpha, hit = np.asarray(alpha).astype(dtype), np.asarray(hit, bool)
    one, tmin = dtype(1), dtype(BR.T_MIN)
    perm = np.argsort(-qd.length, kind="stable")
    len_p = qd.length[perm]
    T = np.where(qd.inside[perm], one, dtype(0)).astype(dtype)
    pix = qd.pix[perm]
    pixels, gaussians, qs = [], [], []
    for pos in range(int(len_p[0]) if qd.Q else 0):
        k = int(np.searchsorted(-len_p, -pos, side="left"))
        idx = qd.off[perm[:k]] + pos
        a = alpha[idx]
        live_hit = hit[idx] & (T[:k] != 0)
        w = (a * T[:k]).astype(dtype)
        test_T = (T[:k] * (one - a).astype(dtype)).astype(dtype)
        ok = test_T >= tmin
        here = live_hit & ok
        q = np.rint((w * dtype(UNIT)).astype(dtype)).astype(np.int64)
        g = np.broadcast_to(qd.pair_id[idx][:, None], q.shape)
        pixels.append(pix[:k][here])
        gaussians.append(g[here])
        qs.append(q[here])
        T[:k] = np.where(live_hit, np.where(ok, test_T, dtype(0)), T[:k])
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)  # noqa: E731
    return cat(pixels), cat(gaussians), cat(qs)


def scatter(contribs, labels, K: int, P: int) -> np.ndarray:
    """int64 [P,K]: the contributions summed by (Gaussian, label of the pixel); labels outside [0, K) are ignored"""
    pix, g, q = contribs
    lab = np.asarray(labels, np.int64).reshape(-1)[pix]
    valid = (lab >= 0) & (lab < K)
    out = np.zeros((P, K), np.int64)
    np.add.at(out, (g[valid], lab[valid]), q[valid])
    return out


def votes(fr: BR.Frame, qd: BR.Quads, alpha, hit, labels, K: int, dtype=np.float32) -> np.ndarray:
    """labels: [H*W] integers.  -> int64 [P,K], the replay's contributions in `dtype` summed as integers"""
    return scatter(contributions(fr, qd, alpha, hit, dtype), labels, K, fr.P)


def loop(events, labels, K: int, P: int, tol: float = 0.0):
    """The same sums from contrib_reference.pixel_loop's events (pixel, Gaussian, w, test_T, contributed), one at a time in
    float64.  -> (votes int64 [P,K], bound float64 [P,K]: the sum over a vote's events of 1 + tol * w * 2^24, what a replay whose
    weights carry a relative error tol may differ by, counts int64 [P,K]: the events per vote)."""
    labels = np.asarray(labels, np.int64).reshape(-1)
    out, cnt = np.zeros((P, K), np.int64), np.zeros((P, K), np.int64)
    bound = np.zeros((P, K))
    for pix, g, w, _test_T, contributed in events:
        l = int(labels[pix])
        if not contributed or not 0 <= l < K:
            continue
        out[g, l] += int(np.rint(w * UNIT))
        bound[g, l] += 1 + tol * w * UNIT
        cnt[g, l] += 1
    return out, bound, cnt


def assign(votes, min_weight=0.0):
    """numpy statement of contrib.assign: (label int64 [P], share float32 [P]) -- the lowest class among those with the most
    votes, found by an explicit scan"""
    votes = np.asarray(votes, np.int64)
    P, K = votes.shape
    label, share = np.full(P, -1, np.int64), np.zeros(P, np.float32)
    for g in range(P):
        total = int(votes[g].sum())
        if total <= 0 or total < min_weight * UNIT:
            continue
        best = 0
        for k in range(1, K):
            if votes[g, k] > votes[g, best]:  # strict: an equal later class does not take over
                best = k
        label[g], share[g] = best, np.float32(np.float64(votes[g, best]) / np.float64(total))
    return label, share


def lift(votes, threshold=0.5, min_weight=0.0):
    votes = np.asarray(votes, np.int64)
    total = votes.sum(1).astype(np.float64)
    return (total > 0) & (total >= min_weight * UNIT) & (votes[:, 1].astype(np.float64) > threshold * total)
