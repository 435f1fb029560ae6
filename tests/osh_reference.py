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


def fit_per_code(lut, counts, HW, w, b, lr=0.01, max_epochs=8000, target_iou=0.9, return_margins=False):
    """Returns dict(epochs, loss, iou, init_iou, trace [epochs, 2], w, b, kink, kink0): the fit in float64; `kink` is the
    smallest distance of any present code's margin to {-1, 0, 1} over the run, `kink0` the smallest |margin| (how far the
    IoU trace is from a flip).  With return_margins also `margins` [epochs + 1, M]: the present codes' margins (in code
    order) under the initial hyperplane and after every step."""
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
    trace, margins = [], [o]
    for ep in range(max_epochs):
        loss = float((P * np.maximum(0, 1 - o) + N * np.maximum(0, 1 + o)).sum() / HW)
        a = (N * (1 + o >= 0) - P * (1 - o >= 0)) / HW
        w -= lr * (a @ z)
        b -= lr * a.sum()
        o = z @ w + b
        margins.append(o)
        if o.size:
            kink = min(kink, np.abs(o[:, None] - np.array([-1.0, 0.0, 1.0])).min())
            kink0 = min(kink0, np.abs(o).min())
        iou = iou_of(o)
        trace.append((loss, iou))
        if ep + 1 == max_epochs or not (iou < target_iou):
            break
    trace = np.array(trace, np.float64)
    res = dict(epochs=len(trace), loss=trace[-1, 0], iou=trace[-1, 1], init_iou=init_iou, trace=trace, w=w, b=b,
               kink=float(kink), kink0=float(kink0))
    if return_margins:
        res["margins"] = np.array(margins, np.float64)
    return res


def iou_flips(a, b):
    """Epochs at which two IoU traces differ (NaN equals NaN)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = min(a.size, b.size)
    a, b = a[:n], b[:n]
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def fit_per_code_f32(lut, counts, HW, w, b, lr=0.01, max_epochs=8000, target_iou=0.9):
    """The statements of fit_per_code in NumPy float32 (plain `@` and `sum`; the IoU from the integer counts): the same
    fields plus `margins`.  Not a model of the kernel -- its summation order is NumPy's, with no per-wave split and no
    FMA: it measures how far an honest fp32 evaluation lies from float64 on a case."""
    f = np.float32
    Pi, Ni = (np.asarray(c, np.int64) for c in counts)
    keep = (Pi + Ni) > 0
    lut = np.asarray(lut, f)[keep]
    Pi, Ni = Pi[keep], Ni[keep]
    P, N = Pi.astype(f), Ni.astype(f)
    z = lut / np.linalg.norm(lut, axis=1, keepdims=True).astype(f) / f(0.3438)
    w = np.asarray(w, f).reshape(-1).copy()
    b, lr, hw, one = f(b), f(lr), f(HW), f(1)
    Ptot = int(Pi.sum())

    def iou_of(o):
        pred = o > 0
        U = Ptot + int(Ni[pred].sum())
        return float("nan") if U == 0 else float(int(Pi[pred].sum())) / float(U)

    o = z @ w + b
    assert o.dtype == f
    init_iou = iou_of(o)
    trace, margins = [], [o]
    for ep in range(max_epochs):
        loss = (P * np.maximum(f(0), one - o) + N * np.maximum(f(0), one + o)).sum() / hw
        a = (N * (one + o >= 0) - P * (one - o >= 0)) / hw
        w = w - lr * (a @ z)
        b = b - lr * a.sum()
        o = z @ w + b
        margins.append(o)
        iou = iou_of(o)
        trace.append((float(loss), iou))
        if ep + 1 == max_epochs or not (iou < target_iou):
            break
    assert w.dtype == f and type(b) is f and o.dtype == f
    trace = np.array(trace, np.float64)
    return dict(epochs=len(trace), loss=trace[-1, 0], iou=trace[-1, 1], init_iou=init_iou, trace=trace, w=w, b=float(b),
                margins=np.array(margins, np.float64))


def kink_of(margins):
    """Smallest distance of any of `margins` to the decision points {-1, 0, 1} (inf for none)."""
    m = np.asarray(margins, np.float64)
    return float(np.abs(m[..., None] - np.array([-1.0, 0.0, 1.0])).min()) if m.size else float("inf")


# ---- the direct cases of tests/test_gpu_osh_direct.py ---------------------------------------------------------------------
# (n_codes, D, present fraction, seed): each shape is the smallest at which a distinct piece of osh_fit_k is exercised.
# Every seed is one at which the case passes the kink guard of tests/test_osh_cpu.py at the shape's longest run.
DIRECT_HW = 4096
DIRECT_BIG_HW = 2 ** 31 - 1
_DIRECT_SHAPES = (
    (1, 1, 1.0, 0), (1, 256, 1.0, 0),        # one code, fifteen waves idle
    (5, 63, 1.0, 0),                         # V = 1, idle lanes
    (15, 256, 1.0, 0), (16, 64, 1.0, 0), (17, 65, 1.0, 0),  # wave boundaries of the code split
    (40, 256, 0.3, 0),                       # M < 16 after compaction
    (37, 100, 1.0, 1),                       # the shape of pin d
    (319, 256, 1.0, 13), (320, 256, 1.0, 13),  # register-path limit
    (321, 256, 1.0, 0),                      # first generic-only size
    (640, 512, 1.0, 0),
    (1000, 256, 0.31, 0),                    # M ~ 310 scattered over 1000 ids
    (1000, 1024, 1.0, 0),                    # V = 16, full LDS
    (1000, 1000, 0.5, 0),                    # V = 16 with a ragged tail
    (999, 33, 1.0, 1),                       # V = 1 at full code count
)
# counts summing to HW = 2^31 - 1: the 32-bit per-wave and 64-bit cross-wave sums
_BIG_COUNTS = ((2 ** 30, 0, 5), (0, 2 ** 30 - 6, 0))
_BIG_SEED = 0


def _epoch_counts(n_codes):
    return (1, 8, 64) if n_codes <= 320 else (1, 8)


# name -> dict(seed, n_codes, D, HW, frac, epochs, b0[, counts])
DIRECT_CASES = {}
for _n, _d, _frac, _seed in _DIRECT_SHAPES:
    for _ep in _epoch_counts(_n):
        DIRECT_CASES[f"{_n}x{_d}_e{_ep}"] = dict(seed=_seed, n_codes=_n, D=_d, HW=DIRECT_HW, frac=_frac, epochs=_ep,
                                                 b0=0.5 if (_n, _d) == (37, 100) else 0.1)
for _ep in _epoch_counts(3):
    DIRECT_CASES[f"3x64_big_e{_ep}"] = dict(seed=_BIG_SEED, n_codes=3, D=64, HW=DIRECT_BIG_HW, frac=1.0, epochs=_ep, b0=0.1,
                                            counts=_BIG_COUNTS)


def make_direct_inputs(seed, n_codes, D, HW, frac, counts=None, alpha=0.2, t=0.3):
    """(lut [n_codes, D] fp32, counts [2, n_codes] int64, w0 [D] fp32) as tests/golden/make_osh_golden.py: make_case draws
    them -- a unit direction u, LUT rows of scale 1.6 / sqrt(D) leaning +-alpha u, a normalised w0 part-aligned with u --
    except that only a drawn subset of the codes (each with probability frac, at least one) is present, interleaved with
    absent ones, and that the counts are drawn per code: every present code has at least one of the HW pixels."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=D)
    u /= np.linalg.norm(u)
    if counts is None:
        pos_code = rng.random(n_codes) < 0.3
        present = rng.random(n_codes) < frac if frac < 1 else np.ones(n_codes, bool)
        if not present.any():
            present[rng.integers(n_codes)] = True
        M = int(present.sum())
        tot = np.zeros(n_codes, np.int64)
        tot[present] = 1 + rng.multinomial(HW - M, np.full(M, 1.0 / M))
        P = rng.binomial(tot, np.where(pos_code, 0.9, 0.05))
        counts = np.stack([P, tot - P])
    else:
        counts = np.asarray(counts, np.int64)
        pos_code = counts[0] > counts[1]
    assert counts.sum() == HW
    lut = (rng.normal(size=(n_codes, D)) * (1.6 / np.sqrt(D)) + alpha * (2 * pos_code - 1)[:, None] * u[None]).astype(np.float32)
    r = rng.normal(size=D)
    r /= np.linalg.norm(r)
    w0 = t * u + (1 - t) * r
    return lut, counts, (w0 / np.linalg.norm(w0)).astype(np.float32)


def direct_case(name):
    """The inputs of DIRECT_CASES[name]: dict(lut, counts, HW, w0, b0, epochs, n_codes, D).  Fits of it run with
    target_iou = 2.0, i.e. exactly `epochs` epochs unless the IoU is NaN."""
    c = DIRECT_CASES[name]
    lut, counts, w0 = make_direct_inputs(c["seed"], c["n_codes"], c["D"], c["HW"], c["frac"], c.get("counts"))
    return dict(lut=lut, counts=counts, HW=c["HW"], w0=w0, b0=c["b0"], epochs=c["epochs"], n_codes=c["n_codes"], D=c["D"])


# the exact-kink cases: w0 = 0, so every margin of the first pass equals b0 in fp32 and float64 alike; one epoch
KINK_SHAPES = ("17x65_e1", "40x256_e1")
KINK_B0 = (1.0, -1.0, 0.0)


def kink_case(shape, b0):
    case = dict(direct_case(shape), b0=float(b0), epochs=1)
    case["w0"] = np.zeros_like(case["w0"])
    return case


def reference_fits(case, lr=0.01):
    """(float64 fit with margins, fp32 restatement) of a direct case."""
    args = (case["lut"], case["counts"], case["HW"], case["w0"], case["b0"])
    kw = dict(lr=lr, max_epochs=case["epochs"], target_iou=2.0)
    return fit_per_code(*args, return_margins=True, **kw), fit_per_code_f32(*args, **kw)


EPS32 = 2.0 ** -23
GUARD_FACTOR = 32  # kink >= 32 x the fp32 restatement's own margin error: the reference alone is far from every decision


def margin_error(r64, r32, first=0):
    """Largest |margin32 - margin64| from pass `first` on."""
    return float(np.abs(r32["margins"][first:] - r64["margins"][first:]).max())


def direct_tolerances(r64, r32, lr=0.01):
    """The bound on |x_gpu - x_f64| per quantity x: 8 d32_x + 8 eps32 scale_x, with d32_x = max |x_f32 - x_f64| of the fp32
    restatement (over elements and epochs) and scale_x = max |x_f64| (for b: max(|b|, lr)).  The factor 8 covers the
    kernel's different but equally legitimate summation order and its FMAs; the additive term the cases where d32 is 0."""
    def tol(d, scale):
        return 8.0 * float(d) + 8.0 * EPS32 * float(scale)
    l64, l32 = r64["trace"][:, 0], r32["trace"][:, 0]
    return dict(trace=tol(np.abs(l32 - l64).max(), np.abs(l64).max()),
                loss=tol(abs(r32["loss"] - r64["loss"]), abs(r64["loss"])),
                w=tol(np.abs(r32["w"] - r64["w"]).max(), np.abs(r64["w"]).max()),
                b=tol(abs(r32["b"] - r64["b"]), max(abs(r64["b"]), lr)))
