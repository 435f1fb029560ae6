"""Test-only float64 restatement of the hyperplane fine-tune (gui/main.py:1673-1763) in its per-code form.

Every pixel's feature is one of the normalised LUT rows, so the per-pixel loop of LinearSVM.step (hinge loss, SGD, IoU)
is a function of P[c] / N[c], the mask-positive / -negative pixel counts of each code.  This is that function in
float64 NumPy: the cross-check of the fixture tests/golden/ref_osh_pins.npz and of csrc/osh.hip's kernel.
"""
from __future__ import annotations

import numpy as np


def counts_of(idx, positive, n_codes):
    """[2, n_codes] int64: pixels of each code with positive != 0 (row 0) and == 0 (row 1)."""
    idx = np.asarray(idx).reshape(-1).astype(np.int64)
    pos = np.asarray(positive).reshape(-1) != 0
    return np.stack([np.bincount(idx[pos], minlength=n_codes), np.bincount(idx[~pos], minlength=n_codes)])


def fit_per_code(lut, counts, HW, w, b, lr=0.01, max_epochs=8000, target_iou=0.9):
    """Returns dict(epochs, loss, iou, init_iou, trace [epochs, 2], w, b, kink, kink0): the fit in float64; `kink` is the
    smallest distance of any present code's margin to {-1, 0, 1} over the run, `kink0` the smallest |margin| (how far the
    IoU trace is from a flip)."""
    P, N = (np.asarray(c, np.float64) for c in counts)
    keep = (P + N) > 0
    lut = np.asarray(lut, np.float64)[keep]
    P, N = P[keep], N[keep]
    z = lut / np.linalg.norm(lut, axis=1, keepdims=True) / 0.3438
    w = np.asarray(w, np.float64).reshape(-1).copy()
    b = float(b)
    Ptot = P.sum()

    def iou_of(o):
        pred = o > 0
        U = Ptot + N[pred].sum()
        return float("nan") if U == 0 else float(P[pred].sum()) / float(U)

    o = z @ w + b
    kink = np.abs(o[:, None] - np.array([-1.0, 0.0, 1.0])).min() if o.size else np.inf
    kink0 = np.abs(o).min() if o.size else np.inf
    init_iou = iou_of(o)
    trace = []
    for ep in range(max_epochs):
        loss = float((P * np.maximum(0, 1 - o) + N * np.maximum(0, 1 + o)).sum() / HW)
        a = (N * (1 + o >= 0) - P * (1 - o >= 0)) / HW
        w -= lr * (a @ z)
        b -= lr * a.sum()
        o = z @ w + b
        if o.size:
            kink = min(kink, np.abs(o[:, None] - np.array([-1.0, 0.0, 1.0])).min())
            kink0 = min(kink0, np.abs(o).min())
        iou = iou_of(o)
        trace.append((loss, iou))
        if ep + 1 == max_epochs or not (iou < target_iou):
            break
    trace = np.array(trace, np.float64)
    return dict(epochs=len(trace), loss=trace[-1, 0], iou=trace[-1, 1], init_iou=init_iou, trace=trace, w=w, b=b,
                kink=float(kink), kink0=float(kink0))


def iou_flips(a, b):
    """Epochs at which two IoU traces differ (NaN equals NaN)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = min(a.size, b.size)
    a, b = a[:n], b[:n]
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())
