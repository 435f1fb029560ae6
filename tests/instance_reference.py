"""goi_hyperplane_amd.instance restated in numpy (tests/test_instance_cpu.py holds it to exact arithmetic, tests/test_gpu_instance.py
holds the kernels to it bit for bit), and the exact side with its error bounds.

THE ORDER (csrc/instance.hip's header, restated): for an instance with members m_0 .. m_{n-1} (ascending row id)

    p = xyz[m_0] (float32; 0 for an empty instance, and every position is the origin without xyz)
    per member r:  w = float64(weight[m_r]) (1 without weights);  d_a = float64(xyz[m_r, a]) - float64(p_a);  t_a = w * d_a
                   terms  W: w | Sd_a: t_a | Sdd_ab: t_a * d_b (xx xy xz yy yz zz) | Sf_c: w * float64(f[m_r, c])
    chunks of 256 consecutive members; in a chunk four accumulators a_0 .. a_3 per quantity, each +0.0 at the start, the member
    at position r goes to a_(r mod 4) in ascending r; the chunk's partial is (a_0 + a_2) + (a_1 + a_3)
    T = +0.0, then T = T + partial in ascending chunk order
    m_a = Sd_a / W; centroid_a = float32(p_a + m_a); cov_ab = float32(Sdd_ab / W - m_a * m_b); feature_c = float32(Sf_c / W);
    wsum = float32(W); W == 0: centroid, cov and feature are 0

every operation in float64, rounded once.  numpy's float64 array arithmetic is IEEE arithmetic element by element, so the 42
quantities of a member are one array here; the loops over chunks and members are explicit.

lo / hi: the smallest / largest coordinate by the total order -0 < +0, NaN skipped, +inf / -inf when nothing is left.

THE BOUNDS (derived, u = 2^-53, n members, w >= 0, first order in u -- n u < 2^-38 for every case here, and every count below is
rounded up by at least one u to pay for the second order).
  A sum of n terms in ANY order is off by at most (n - 1) u sum|t|.  A term w * f of two float32 is exact in float64, so
      |Sf^ - Sf| <= (n - 1) u sum|w f|,    |W^ - W| <= (n - 1) u W,    and the quotient adds u:
      |mean64 - mean| <= (2 n - 1) u sum|w f| / W <= (n + 2) 2^-52 sum|w f| / W
  and the one rounding to float32 adds 2^-24 |mean| (plus 2^-150, half the smallest denormal):
      |got - exact| <= 2^-24 |exact| + (n + 2) 2^-52 sum|w f| / W + 2^-150                                              (mean_bound)
  centroid = p + Sd / W: d = x - p and t = w * d are rounded (2 u per term), so the same count holds with f := x - p
  ((n - 1) + 2 + (n - 1) + 1 = 2 n + 1 <= 2 n + 4), and the addition of p adds u |c|:
      |got - c| <= 2^-24 |c| + (n + 2) 2^-52 sum|w (x - p)| / W + 2^-52 |c| + 2^-150
  cov_ab = Sdd_ab / W - m_a m_b (an identity in exact arithmetic, whatever p).  With A = sum|w d_a d_b| / W and
  M_a = sum|w d_a| / W >= |m_a|: a term of Sdd carries four roundings, so Sdd^ / W^ is off by (4 + (n - 1) + (n - 1) + 1) u A =
  (2 n + 3) u A; m^_a is off by (2 n + 1) u M_a, the product by ((2 n + 1) 2 + 1) u M_a M_b = (4 n + 3) u M_a M_b; the subtraction
  adds u (A + M_a M_b):
      |got - cov| <= 2^-24 |cov| + (n + 2) 2^-52 (A + 2 M_a M_b) + 2^-150                                              (cov_bound)
THE EXACT SIDE is fractions.Fraction throughout (a float is a dyadic rational): sum w, sum w x, sum w x x^T and sum w f over the
RAW positions -- no pivot -- so it shares nothing with the restatement.  An instance with a non-finite input on an axis has no
exact value there (None); the restatement must then give NaN.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

CHUNK = 256
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # cov: xx xy xz yy yz zz
U52 = 2.0 ** -52
TINY = 2.0 ** -150


def members(label, K):
    """(ptr int32 [K+1], rows int32 [P]) by a stable argsort of key = label inside [0, K), K outside"""
    label = np.asarray(label, np.int32)
    P = label.shape[0]
    key = np.where((label >= 0) & (label < K), label.astype(np.int64), K)
    order = np.argsort(key, kind="stable").astype(np.int32)
    counts = np.bincount(key, minlength=K + 1)[:K]
    ptr = np.zeros(K + 1, np.int64)
    np.cumsum(counts, out=ptr[1:])
    rows = np.where(np.arange(P) < ptr[K], order, -1).astype(np.int32)
    return ptr.astype(np.int32), rows


def _key(v):
    """the order-preserving integer key of float32 values (wave_util.h: ord_enc): -0 < +0"""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)


def _unkey(k):
    k = np.asarray(k, np.int64)
    b = np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k & 0xFFFFFFFF)
    return b.astype(np.uint32).view(np.float32)


def box(x):
    """(lo, hi) of float32 values: NaN skipped, -0 < +0, (+inf, -inf) when nothing is left"""
    x = np.asarray(x, np.float32)
    x = x[~np.isnan(x)]
    if x.size == 0:
        return np.float32(np.inf), np.float32(-np.inf)
    k = _key(x)
    return _unkey(k.min())[()], _unkey(k.max())[()]


def stats(ptr, rows, xyz, features=None, weight=None, hit=None):
    """dict(n, hits, wsum, centroid, lo, hi, cov, feature) in the documented order and roundings (module docstring)"""
    K = len(ptr) - 1
    P = len(rows)
    S = 0 if features is None else features.shape[1]
    out = dict(n=np.zeros(K, np.int32), hits=np.zeros((K, 8), np.int32), wsum=np.zeros(K, np.float32),
               centroid=np.zeros((K, 3), np.float32), lo=np.zeros((K, 3), np.float32), hi=np.zeros((K, 3), np.float32),
               cov=np.zeros((K, 6), np.float32), feature=None if features is None else np.zeros((K, S), np.float32))
    pos = np.zeros((P, 3), np.float32) if xyz is None else np.asarray(xyz, np.float32)
    ia, ib = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            m = np.asarray(rows[ptr[k]:ptr[k + 1]], np.int64)
            n = len(m)
            out["n"][k] = n
            p = pos[m[0]].astype(np.float64) if n else np.zeros(3)
            total = np.zeros(10 + S)  # W | Sd 3 | Sdd 6 | Sf S
            for c0 in range(0, n, CHUNK):
                acc = np.zeros((4, 10 + S))
                for r in range(c0, min(c0 + CHUNK, n)):
                    i = m[r]
                    w = np.float64(1.0 if weight is None else weight[i])
                    d = pos[i].astype(np.float64) - p
                    t = w * d
                    term = np.empty(10 + S)
                    term[0] = w
                    term[1:4] = t
                    term[4:10] = t[ia] * d[ib]
                    if S:
                        term[10:] = w * features[i].astype(np.float64)
                    acc[r & 3] = acc[r & 3] + term
                total = total + ((acc[0] + acc[2]) + (acc[1] + acc[3]))
            W = total[0]
            out["wsum"][k] = np.float32(W)
            if W != 0.0:
                mean = total[1:4] / W
                out["centroid"][k] = (p + mean).astype(np.float32)
                out["cov"][k] = (total[4:10] / W - mean[ia] * mean[ib]).astype(np.float32)
                if S:
                    out["feature"][k] = (total[10:] / W).astype(np.float32)
            for a in range(3):
                out["lo"][k, a], out["hi"][k, a] = box(pos[m, a])
            if hit is not None:
                h = np.asarray(hit)[m].astype(np.uint8)
                out["hits"][k] = [int(((h >> b) & 1).sum()) for b in range(8)]
    return out


def fraction_of(min_fraction):
    """instance.fraction_of restated: (num, den)"""
    q = Fraction(repr(min_fraction)) if isinstance(min_fraction, float) else Fraction(min_fraction)
    q = q.limit_denominator(2 ** 32 - 1)
    return q.numerator, q.denominator


def vote(n, hits, min_fraction=0.5, min_hits=1, bit=0):
    """bool [K]: hits >= min_hits and hits * den >= num * n, in Python integers"""
    num, den = fraction_of(min_fraction)
    return np.array([int(h) >= min_hits and int(h) * den >= num * int(c) for h, c in zip(hits[:, bit], n)], bool)


def rows_of(label, keep):
    """bool [P]: keep[label] of a row whose label is inside [0, K)"""
    K = len(keep)
    return np.array([bool(0 <= int(l) < K and keep[int(l)]) for l in label], bool)


def select(label, K, hit, min_fraction=0.5, min_hits=1):
    ptr, rows = members(label, K)
    st = stats(ptr, rows, None, hit=hit)
    return rows_of(label, vote(st["n"], st["hits"], min_fraction, min_hits))


# ---- the exact side and the bounds ---------------------------------------------------------------------------------------------------
def _fr(v):
    return Fraction(float(v))


def exact(ptr, rows, xyz, features=None, weight=None):
    """Per instance a dict of Fractions -- W, centroid [3], cov [6], feature [S], and the magnitudes the bounds need: absd [3]
    = sum|w (x - p)| / W, absdd [6] = sum|w d_a d_b| / W, absf [S] = sum|w f| / W -- or None in place of a value whose inputs
    are not all finite.  W == 0: zeros, as documented."""
    K = len(ptr) - 1
    S = 0 if features is None else features.shape[1]
    res = []
    for k in range(K):
        m = [int(i) for i in rows[ptr[k]:ptr[k + 1]]]
        w = [Fraction(1) if weight is None else _fr(weight[i]) for i in m]
        W = sum(w, Fraction(0))
        e = dict(n=len(m), W=W, centroid=[Fraction(0)] * 3, cov=[Fraction(0)] * 6, feature=[Fraction(0)] * S,
                 absd=[Fraction(0)] * 3, absdd=[Fraction(0)] * 6, absf=[Fraction(0)] * S)
        res.append(e)
        if W == 0:
            continue
        finite = [bool(np.all(np.isfinite(xyz[m, a]))) for a in range(3)]
        x = [[_fr(xyz[i, a]) if finite[a] else Fraction(0) for i in m] for a in range(3)]
        p = [x[a][0] for a in range(3)]
        c = [sum((wi * xi for wi, xi in zip(w, x[a])), Fraction(0)) / W for a in range(3)]
        for a in range(3):
            e["centroid"][a] = c[a] if finite[a] else None
            e["absd"][a] = sum((abs(wi * (xi - p[a])) for wi, xi in zip(w, x[a])), Fraction(0)) / W
        for q, (a, b) in enumerate(PAIRS):
            if not (finite[a] and finite[b]):
                e["cov"][q] = None
                continue
            e["cov"][q] = sum((wi * xa * xb for wi, xa, xb in zip(w, x[a], x[b])), Fraction(0)) / W - c[a] * c[b]
            e["absdd"][q] = sum((abs(wi * (xa - p[a]) * (xb - p[b])) for wi, xa, xb in zip(w, x[a], x[b])), Fraction(0)) / W
        for ch in range(S):
            f = [_fr(features[i, ch]) for i in m]
            e["feature"][ch] = sum((wi * fi for wi, fi in zip(w, f)), Fraction(0)) / W
            e["absf"][ch] = sum((abs(wi * fi) for wi, fi in zip(w, f)), Fraction(0)) / W
    return res


def mean_bound(n, value, magnitude, extra=0.0):
    """|got - exact| for a weighted mean: value its exact value, magnitude sum|w f| / W (module docstring)"""
    return 2.0 ** -24 * abs(float(value)) + (n + 2) * U52 * float(magnitude) + extra + TINY


def centroid_bound(n, value, magnitude):
    return mean_bound(n, value, magnitude, U52 * abs(float(value)))


def cov_bound(n, value, absdd, absd_a, absd_b):
    return 2.0 ** -24 * abs(float(value)) + (n + 2) * U52 * (float(absdd) + 2.0 * float(absd_a) * float(absd_b)) + TINY
