"""numpy restatement of goi_hyperplane_amd.grouping's mask-contrast loss (csrc/grouping.hip).

    quantum(feat, max_abs=None)                  -> (e, q): the smallest e with max|f| < 2^e over the whole map (0 for zeros), q = 40 - e
    sums(feat, labels, K, max_abs=None)          -> (count int64 [K], qsum int64 [K,S], qexp, status): exact integers
    terms(feat, labels, K, ...)                  -> dict(loss, intra, inter, grad [S,H,W], count, qsum, qexp, status, a, mu, g): float64
    twin(feat, labels, K, ...)                   -> dict(loss, intra, inter, grad) as float32 arithmetic gives them: the error yardstick
    definition(feat, labels, K, ...)             -> (loss, grad): float64 autograd of the definition on the CPU

`terms` is the definition with the means taken from the integer sums (mu = qsum * 2^-q / n, as the kernels do: two masks made of
the same multiset of pixels then have d == 0 exactly) and the closed-form gradient alpha f + beta in its centred form.  `twin`
follows the torch route -- index_add, means, gather, pair block -- with every array and every sum in float32; its distance to
`terms` on a case is what float32 arithmetic costs there, and the GPU is held to 8 times that (or 64 ulps).
"""
from __future__ import annotations

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
QBITS = 40


def quantum(feat, max_abs=None):
    top = float(np.abs(feat).max()) if max_abs is None else float(np.float32(max_abs))
    if top == 0.0:
        return 0, QBITS
    _, e = np.frexp(top)  # top = m * 2^e, 0.5 <= m < 1: top < 2^e and 2^(e-1) <= top
    return int(e), QBITS - int(e)


def _inside(labels, K):
    lab = labels.reshape(-1).astype(np.int64)
    return lab, (lab >= 0) & (lab < K)


def sums(feat, labels, K, max_abs=None):
    S = feat.shape[0]
    e, q = quantum(feat, max_abs)
    lab, ok = _inside(labels, K)
    f = feat.reshape(S, -1).T.astype(np.float64)[ok]
    big = ~(np.abs(f) < 2.0 ** e)
    v = np.where(big, np.copysign(2.0 ** QBITS, f), np.rint(f * 2.0 ** q)).astype(np.int64)
    count = np.bincount(lab[ok], minlength=K).astype(np.int64)[:K] if K else np.zeros(0, np.int64)
    qsum = np.zeros((K, S), np.int64)
    order = np.argsort(lab[ok], kind="stable")
    if order.size:
        sl, sv = lab[ok][order], v[order]
        starts = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
        qsum[sl[starts]] = np.add.reduceat(sv, starts, axis=0)
    return count, qsum, q, int(bool(big.any()))


def terms(feat, labels, K, margin=1.0, w_intra=1.0, w_inter=1.0, balance="pixel", max_abs=None):
    S, H, W = feat.shape
    count, qsum, q, status = sums(feat, labels, K, max_abs)
    lab, ok = _inside(labels, K)
    live = count > 0
    M, N = int(live.sum()), int(count.sum())
    n = np.maximum(count, 1).astype(np.float64)
    mu = np.where(live[:, None], qsum.astype(np.float64) * 2.0 ** -q / n[:, None], 0.0)
    a = np.zeros(K)
    if M:
        a[live] = 1.0 / N if balance == "pixel" else 1.0 / (M * n[live])
    g, inter = np.zeros((K, S)), 0.0
    if M > 1:
        ids = np.flatnonzero(live)
        diff = mu[ids][:, None, :] - mu[ids][None, :, :]
        d2 = (diff * diff).sum(-1)
        d = np.sqrt(d2)
        off = ~np.eye(M, dtype=bool)
        pair = np.where(d2 == 0, margin * margin, np.maximum(0.0, margin - d) ** 2)
        inter = float(pair[off].sum() / (M * (M - 1)))
        pull = off & (d2 > 0) & (d < margin)
        coef = np.where(pull, (margin - d) / np.where(pull, d, 1.0), 0.0)
        g[ids] = -4.0 / (M * (M - 1)) * (coef[:, :, None] * diff).sum(1)
    f = feat.reshape(S, -1).T.astype(np.float64)
    grad = np.zeros((H * W, S))
    lo = lab[ok]
    dev = f[ok] - mu[lo]
    intra = float((a[lo] * (dev * dev).sum(-1)).sum())
    grad[ok] = 2.0 * w_intra * a[lo][:, None] * dev + (w_inter * g / n[:, None])[lo]
    return dict(loss=w_intra * intra + w_inter * inter, intra=intra, inter=inter, grad=np.ascontiguousarray(grad.T).reshape(S, H, W),
                count=count, qsum=qsum, qexp=q, status=status, a=a, mu=mu, g=g, M=M, N=N)


def twin(feat, labels, K, margin=1.0, w_intra=1.0, w_inter=1.0, balance="pixel"):
    """the torch route in float32: index_add_ (sequential float32 adds), means, gather, pair block, the gradient autograd returns"""
    f32 = np.float32
    S, H, W = feat.shape
    lab, ok = _inside(labels, K)
    f = np.ascontiguousarray(feat.reshape(S, -1).T)[ok].astype(f32)
    lo = lab[ok]
    total, count = np.zeros((K, S), f32), np.zeros(K, f32)
    np.add.at(total, lo, f)
    np.add.at(count, lo, f32(1))
    live = count > 0
    M, N = int(live.sum()), f32(count.sum(dtype=f32))
    n = np.maximum(count, f32(1))
    mu = (total / n[:, None]).astype(f32)
    a = np.zeros(K, f32)
    if M:
        a[live] = f32(1) / N if balance == "pixel" else f32(1) / (f32(M) * n[live])
    g, inter = np.zeros((K, S), f32), f32(0)
    margin = f32(margin)
    if M > 1:
        ids = np.flatnonzero(live)
        diff = (mu[ids][:, None, :] - mu[ids][None, :, :]).astype(f32)
        d2 = (diff * diff).sum(-1, dtype=f32)
        d = np.sqrt(d2, dtype=f32)
        off = ~np.eye(M, dtype=bool)
        pair = np.where(d2 == 0, margin * margin, np.maximum(f32(0), margin - d) ** 2).astype(f32)
        inter = f32(pair[off].sum(dtype=f32) / f32(M * (M - 1)))
        pull = off & (d2 > 0) & (d < margin)
        coef = np.where(pull, (margin - d) / np.where(pull, d, f32(1)), f32(0)).astype(f32)
        g[ids] = (f32(-4.0 / (M * (M - 1))) * (coef[:, :, None] * diff).sum(1, dtype=f32)).astype(f32)
    dev = (f - mu[lo]).astype(f32)
    intra = f32((a[lo] * (dev * dev).sum(-1, dtype=f32)).sum(dtype=f32))
    grad = np.zeros((H * W, S), f32)
    grad[ok] = f32(2) * f32(w_intra) * a[lo][:, None] * dev + (f32(w_inter) * g / n[:, None])[lo]
    return dict(loss=f32(f32(w_intra) * intra + f32(w_inter) * inter), intra=intra, inter=inter,
                grad=np.ascontiguousarray(grad.T).reshape(S, H, W))


def definition(feat, labels, K, margin=1.0, w_intra=1.0, w_inter=1.0, balance="pixel"):
    """float64 autograd of the definition (the exact means of the float64 features, not the quantised ones) -> (loss, grad)"""
    import torch
    S, H, W = feat.shape
    f = torch.tensor(feat.reshape(S, -1).T.astype(np.float64), requires_grad=True)
    lab, ok = _inside(labels, K)
    okt, lo = torch.from_numpy(ok), torch.from_numpy(lab[ok])
    count = torch.zeros(K, dtype=torch.float64).index_add_(0, lo, torch.ones(lo.shape[0], dtype=torch.float64))
    live = count > 0
    M, N = int(live.sum()), float(count.sum())
    if M == 0:
        return 0.0, np.zeros((S, H, W))
    n = count.clamp(min=1)
    mu = torch.zeros((K, S), dtype=torch.float64).index_add_(0, lo, f[okt]) / n[:, None]
    a = torch.where(live, torch.full_like(n, 1.0 / N) if balance == "pixel" else 1.0 / (M * n), torch.zeros_like(n))
    intra = (a[lo] * ((f[okt] - mu[lo]) ** 2).sum(-1)).sum()
    inter = torch.zeros((), dtype=torch.float64)
    if M > 1:
        m = mu[live]
        d2 = ((m[:, None, :] - m[None, :, :]) ** 2).sum(-1)
        off = ~torch.eye(M, dtype=torch.bool)
        d = torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2)))
        pair = torch.where(d2 > 0, torch.clamp(margin - d, min=0) ** 2, torch.full_like(d2, margin * margin))
        inter = pair[off].sum() / (M * (M - 1))
    total = w_intra * intra + w_inter * inter
    total.backward()
    return float(total.detach()), np.ascontiguousarray(f.grad.numpy().T).reshape(S, H, W)
