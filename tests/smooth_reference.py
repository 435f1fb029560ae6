"""What goi_hyperplane_amd.smooth must compute, in numpy (csrc/smooth.hip).

Every function takes a `dtype`:
    np.float32   every operation in the documented order, one rounding each: the BIT-LEVEL reference of the kernels;
    np.float64   the same formulas in float64 from the same float32 inputs: the truth the error bounds are measured against.

    L = (1 / N_E) sum over counting edges (i, m) of w[i,m] sum_c (f[i,c] - f[j,c])^2,  j = idx[i,m]
    entry (i, m) is an edge iff 0 <= idx[i,m] < P; an edge counts iff rows[i] != 0; N_E = the number of counting edges.

Orders (float32):
  gradient element (a, c): acc = 0; over row a's k slots in slot order, then over its in-list in stored order (ascending flat
      edge number), for every counting edge t = f[a,c] - f[other,c], acc = acc + w * t; then acc * scale, scale = float32(2 / N_E).
  row loss: per edge, lane l < 16 holds q_l = t_l^2 (+ t_{l+16}^2 when S > 16; 0 for a channel >= S), the 16 lanes are summed
      pairwise (offsets 8, 4, 2, 1), r = r + w * q in slot order; rows are summed in float64 and L = float32(sum / N_E).
  diffusion: W = W + w and acc_c = acc_c + w * f[j,c] over a row's edges in slot order, m_c = acc_c / W,
      out = f + lam * (m_c - f).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def gamma(n):
    """Higham's gamma_n for float32: the relative error bound of a chain of n roundings"""
    return n * U / (1.0 - n * U)


def edge_mask(idx):
    P = idx.shape[0]
    return (idx >= 0) & (idx < P)


def counting_mask(idx, rows=None):
    m = edge_mask(idx)
    if rows is not None:
        m &= (np.asarray(rows) != 0)[:, None]
    return m


def transpose(idx):
    """-> (in_ptr int32 [P+1], in_edge int32 [P*k]): the kept flat edge numbers in ascending (target, edge) order, -1 behind"""
    P, k = idx.shape
    flat = idx.reshape(-1).astype(np.int64)
    kept = np.flatnonzero((flat >= 0) & (flat < P))
    order = kept[np.argsort(flat[kept], kind="stable")]
    in_edge = np.full(P * k, -1, np.int32)
    in_edge[:len(order)] = order
    in_ptr = np.zeros(P + 1, np.int32)
    in_ptr[1:] = np.cumsum(np.bincount(flat[kept], minlength=P))
    return in_ptr, in_edge


def transpose_double_loop(idx):
    """the same by the definition: for every target, every entry in flat order"""
    P, k = idx.shape
    in_ptr, in_edge = [0], []
    for a in range(P):
        for i in range(P):
            for m in range(k):
                if idx[i, m] == a:
                    in_edge.append(i * k + m)
        in_ptr.append(len(in_edge))
    return (np.array(in_ptr, np.int32), np.array(in_edge + [-1] * (P * k - len(in_edge)), np.int32).reshape(P * k))


def _terms(idx, weight, rows, T, visit):
    """Walks every gradient term in the documented order, vectorised over the rows: visit(rows_a, other, w) is called once per
    out-slot with the rows whose slot counts, then once per in-list rank with the rows whose in-list is that long and whose edge
    at that rank counts."""
    P, k = idx.shape
    cnt = counting_mask(idx, rows)
    for m in range(k):
        a = np.flatnonzero(cnt[:, m])
        if len(a):
            visit(a, idx[a, m], None if weight is None else weight[a, m])
    in_ptr, in_edge = T
    deg = np.diff(in_ptr)
    live = np.flatnonzero(deg > 0)
    wflat = None if weight is None else weight.reshape(-1)
    for r in range(int(deg.max()) if P else 0):
        live = live[deg[live] > r]
        e = in_edge[in_ptr[live] + r]
        src = e // k
        ok = np.ones(len(live), bool) if rows is None else np.asarray(rows)[src] != 0
        if ok.any():
            visit(live[ok], src[ok], None if wflat is None else wflat[e[ok]])


def n_edges(idx, rows=None):
    return int(counting_mask(idx, rows).sum())


def loss_and_grad(f, idx, weight=None, rows=None, dtype=np.float32, transposed=None):
    """-> (L, dL/df [P,S], N_E) in `dtype` (module docstring for the float32 orders)"""
    P, S = f.shape
    k = idx.shape[1]
    T = transposed if transposed is not None else transpose(idx)
    F = f.astype(dtype)
    W = None if weight is None else weight.astype(dtype)
    ne = n_edges(idx, rows)
    acc = np.zeros((P, S), dtype)

    def add(a, other, w):
        t = F[a] - F[other]
        acc[a] = acc[a] + (t if w is None else w[:, None] * t)

    _terms(idx, W, rows, T, add)
    if ne == 0:
        return dtype(0), np.zeros((P, S), dtype), 0
    grad = acc * dtype(2.0 / ne)

    cnt = counting_mask(idx, rows)
    row_loss = np.zeros(P, dtype)
    pad = np.zeros((P, 32), dtype)
    pad[:, :S] = F
    for m in range(k):
        a = np.flatnonzero(cnt[:, m])
        if not len(a):
            continue
        t = pad[a] - pad[idx[a, m]]
        q = t[:, :16] * t[:, :16]
        if S > 16:
            q = q + t[:, 16:] * t[:, 16:]
        for half in (8, 4, 2, 1):
            q = q[:, :half] + q[:, half:]
        q = q[:, 0]
        row_loss[a] = row_loss[a] + (q if W is None else W[a, m] * q)
    return dtype(row_loss.astype(np.float64).sum() / ne), grad, ne


def loss_chain(S, k):
    """n of the loss bound gamma(n) L: the longest chain of float32 roundings one row's loss goes through, every term being
    non-negative.  t = a - b is rounded and then squared (2), the square (1), the second channel's addition (1 when S > 16), the
    pairwise sum over min(S, 16) lanes that hold a channel (ceil(log2)), the product with w (1), the k additions of the row (k),
    the final rounding of the float64 quotient to float32 (1), and 1 for the float64 sums (P k 2^-53 is far below 2^-24)."""
    lanes = min(S, 16)
    return 2 + 1 + (1 if S > 16 else 0) + int(np.ceil(np.log2(lanes))) + 1 + k + 1 + 1


def grad_bound(f, idx, weight=None, rows=None, transposed=None):
    """[P,S] float64: gamma(n_a) |scale| sum |w t| per element, n_a = (terms of row a) + 5: t and w * t are rounded once each and
    go through at most (terms) additions (terms + 2), the scale is a rounded float64 quotient (2), the last product (1)."""
    P, S = f.shape
    T = transposed if transposed is not None else transpose(idx)
    F = f.astype(np.float64)
    W = None if weight is None else weight.astype(np.float64)
    mag = np.zeros((P, S))
    terms = np.zeros(P, np.int64)

    def add(a, other, w):
        t = np.abs(F[a] - F[other])
        mag[a] += t if w is None else np.abs(w)[:, None] * t
        terms[a] += 1

    _terms(idx, W, rows, T, add)
    ne = n_edges(idx, rows)
    if ne == 0:
        return np.zeros((P, S))
    return gamma(terms + 5)[:, None] * (2.0 / ne) * mag


def weight_degree(idx, weight=None, rows=None):
    """d_max: the largest per-row sum of in- plus out-edge weights over the counting edges (the Hessian's largest eigenvalue is at
    most 4 d_max / N_E: it is (2 / N_E) times twice a weighted graph Laplacian, whose eigenvalues are at most 2 d_max)"""
    P, k = idx.shape
    cnt = counting_mask(idx, rows)
    w = np.ones((P, k)) if weight is None else weight.astype(np.float64)
    d = np.where(cnt, w, 0.0).sum(axis=1)
    np.add.at(d, idx[cnt], w[cnt])
    return float(d.max()) if P else 0.0


def diffuse(f, idx, weight=None, fixed=None, lam=1.0, iterations=1, dtype=np.float32):
    """-> [P,S] in `dtype` after `iterations` Jacobi steps; fixed rows, rows without an edge and rows with W == 0 are copied"""
    P, S = f.shape
    k = idx.shape[1]
    cur = f.astype(dtype)
    edge = edge_mask(idx)
    W = None if weight is None else weight.astype(dtype)
    lam = dtype(lam)
    for _ in range(iterations):
        wsum = np.zeros(P, dtype)
        acc = np.zeros((P, S), dtype)
        for m in range(k):
            a = np.flatnonzero(edge[:, m])
            if not len(a):
                continue
            w = np.ones(len(a), dtype) if W is None else W[a, m]
            wsum[a] = wsum[a] + w
            acc[a] = acc[a] + w[:, None] * cur[idx[a, m]]
        move = edge.any(axis=1) & (wsum != 0)
        if fixed is not None:
            move &= np.asarray(fixed) == 0
        nxt = cur.copy()
        a = np.flatnonzero(move)
        mean = acc[a] / wsum[a][:, None]
        nxt[a] = cur[a] + lam * (mean - cur[a])
        cur = nxt
    return cur
