"""Neighbour consistency of per-Gaussian features on the k-NN graph (csrc/smooth.hip over the C ABI).

    transpose(idx)                                                       -> (in_ptr int32 [P+1], in_edge int32 [P*k])
    loss(features, idx, weight=None, rows=None, transposed=None)          -> 0-d float32, differentiable in `features`
    loss_terms(features, idx, weight=None, rows=None, transposed=None)    -> (loss, n_edges int64 0-d)
    gaussian_weights(dist2, sigma)                                        -> float32 [P,k]
    diffuse(features, idx, weight=None, fixed=None, lam=1.0, iterations=1) -> float32 [P,S]
    complete_features(xyz, features, known, k=8, iterations=8, selection=None) -> float32 [P,S]

The semantic stage trains a Gaussian's feature only through the pixels that blend it; a Gaussian no pixel blends keeps the
feature it was initialised with, and the viewer decodes it all the same.  Two repairs over `knn.graph(xyz, k)`:

DURING TRAINING the regulariser

    L = (1 / N_E) * sum over counting edges (i, m) of  w[i,m] * sum_c (f[i,c] - f[idx[i,m],c])^2

where entry (i, m) is an edge iff 0 <= idx[i,m] < P (the -1 tails of a graph and ids out of range are skipped), an edge counts
iff rows[i] != 0, and N_E is the number of counting edges (L = 0 and a zero gradient when there is none).  Its gradient needs
the transpose of the graph -- who points at me -- which makes it a gather: no float atomics, the same bits on every call.  The
transpose knows neither `weight` nor `rows`: build it once for a run (the semantic stage has frozen geometry).

AFTER TRAINING `diffuse` / `complete_features`, the continuous counterpart of `knn.complete_labels`: Jacobi steps that pull every
row that is not `fixed` towards the weighted mean of its neighbours.

float32 tensors on a ROCm GPU only; there is no CPU fallback.  Nothing here synchronises the host: N_E stays on the device.
"""
from __future__ import annotations

import math

import torch

from . import _lib, knn
from ._lib import check, ptr, stream

_NO_CPU = "goi_hyperplane_amd.smooth: tensors must live on a ROCm GPU; there is no CPU fallback"
S_MAX = 32            # goi_knn_smooth_loss / goi_knn_diffuse: 1 <= S <= 32
MAX_ENTRIES = 2 ** 30  # P * k below this


def _tensor(t, who, what, dtypes):
    """a tensor of one of `dtypes`; where it lives is looked at last (_on_gpu), so that a wrong dtype or shape is named as such"""
    if not torch.is_tensor(t):
        raise TypeError(f"smooth.{who}: {what} must be a tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"smooth.{who}: {what} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")
    return t


def _on_gpu(who, **tensors):
    """every given tensor on ONE ROCm GPU (None: not given)"""
    given = {name: t for name, t in tensors.items() if t is not None}
    if any(not t.is_cuda for t in given.values()):
        raise RuntimeError(_NO_CPU)
    first = next(iter(given.values())).device
    for name, t in given.items():
        if t.device != first:
            raise ValueError(f"smooth.{who}: {name} is on {t.device}, expected {first}")


def _idx(idx, who, P=None):
    """int32 [P,k], k >= 1, P * k < 2^30, contiguous"""
    idx = _tensor(idx, who, "idx", (torch.int32,))
    if idx.dim() != 2 or idx.shape[1] < 1:
        raise ValueError(f"smooth.{who}: idx must have shape (P, k) with k >= 1")
    if P is not None and idx.shape[0] != P:
        raise ValueError(f"smooth.{who}: idx must have {P} rows, one per row of features")
    if idx.shape[0] * idx.shape[1] >= MAX_ENTRIES:
        raise ValueError(f"smooth.{who}: need P * k < 2^30")
    return idx.contiguous()


def _features(f, who):
    f = _tensor(f, who, "features", (torch.float32,))
    if f.dim() != 2 or not 1 <= f.shape[1] <= S_MAX:
        raise ValueError(f"smooth.{who}: features must have shape (P, S) with 1 <= S <= {S_MAX}")
    return f


def _weight(w, idx, who):
    if w is None:
        return None
    w = _tensor(w, who, "weight", (torch.float32,))
    if w.shape != idx.shape:
        raise ValueError(f"smooth.{who}: weight must have idx's shape {tuple(idx.shape)}")
    return w.detach().contiguous()


def _bytes(m, P, who, what):
    """bool (or uint8) [P] -> contiguous uint8 (a view of a contiguous bool: no copy); None stays None"""
    if m is None:
        return None
    m = _tensor(m, who, what, (torch.bool, torch.uint8))
    if tuple(m.shape) != (P,):
        raise ValueError(f"smooth.{who}: {what} must have shape ({P},)")
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _transposed(T, idx, who):
    if not isinstance(T, (tuple, list)) or len(T) != 2:
        raise TypeError(f"smooth.{who}: transposed must be the pair transpose(idx) returned")
    P, k = int(idx.shape[0]), int(idx.shape[1])
    in_ptr = _tensor(T[0], who, "transposed[0]", (torch.int32,))
    in_edge = _tensor(T[1], who, "transposed[1]", (torch.int32,))
    if tuple(in_ptr.shape) != (P + 1,) or tuple(in_edge.shape) != (P * k,):
        raise ValueError(f"smooth.{who}: transposed must have shapes ({P + 1},) and ({P * k},)")
    return in_ptr.contiguous(), in_edge.contiguous()


def transpose(idx):
    """-> (in_ptr int32 [P+1], in_edge int32 [P*k]): who points at every row.  in_edge holds the flat edge numbers e = i * k + m
    of the edges (0 <= idx[e] < P) in ascending (idx[e], e) order, those that point at row a in in_edge[in_ptr[a] : in_ptr[a+1]];
    in_ptr[P] is the number of edges and in_edge is -1 from there on.  From e the source row is e // k and the weight
    weight.view(-1)[e].  Built from all edges, whatever `rows` and `weight` a loss is later called with.  Asynchronous, no
    read-back."""
    idx = _idx(idx, "transpose")
    _on_gpu("transpose", idx=idx)
    lib = _lib.load()
    dev = idx.device
    P, k = int(idx.shape[0]), int(idx.shape[1])
    with torch.cuda.device(dev):
        in_ptr = torch.empty((P + 1,), dtype=torch.int32, device=dev)
        in_edge = torch.empty((P * k,), dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.goi_knn_transpose_workspace_bytes(P, k), dev)
        check(lib.goi_knn_transpose(P, k, ptr(idx), ptr(in_ptr), ptr(in_edge), ptr(ws), stream(dev)))
    return in_ptr, in_edge


def _forward(f, idx, weight, rows, T, want_grad):
    """-> (loss float32 0-d, n_edges int64 0-d, dL/dfeatures [P,S] or None)"""
    lib = _lib.load()
    dev = f.device
    P, S, k = int(f.shape[0]), int(f.shape[1]), int(idx.shape[1])
    with torch.cuda.device(dev):
        loss = torch.empty((), dtype=torch.float32, device=dev)
        n_edges = torch.empty((), dtype=torch.int64, device=dev)
        grad = torch.empty((P, S), dtype=torch.float32, device=dev) if want_grad else None
        ws = _lib.workspace(lib.goi_knn_smooth_loss_workspace_bytes(P), dev)
        check(lib.goi_knn_smooth_loss(P, S, k, ptr(f), ptr(idx), ptr(weight), ptr(rows), ptr(T[0]) if want_grad else None,
                                      ptr(T[1]) if want_grad else None, ptr(loss), ptr(n_edges), ptr(grad), ptr(ws), stream(dev)))
    return loss, n_edges, grad


class _SmoothLoss(torch.autograd.Function):
    """The gradient is formed by the forward (one pass over the graph serves both) and saved; the backward is one multiply by
    the upstream scalar on the device.  (loss_terms comes here only when a gradient is wanted: without one none is allocated.)"""

    @staticmethod
    def forward(ctx, features, idx, weight, rows, T):
        loss, n_edges, grad = _forward(features.detach().contiguous(), idx, weight, rows, T, True)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(n_edges)
        return loss, n_edges

    @staticmethod
    def backward(ctx, g_loss, _g_n):
        (grad,) = ctx.saved_tensors
        return grad * g_loss, None, None, None, None


def loss_terms(features, idx, weight=None, rows=None, transposed=None):
    """-> (loss float32 0-d, n_edges int64 0-d), both on the device; `loss` is differentiable in `features`.  See loss()."""
    f = _features(features, "loss")
    idx = _idx(idx, "loss", int(f.shape[0]))
    weight = _weight(weight, idx, "loss")
    rows = _bytes(rows, int(f.shape[0]), "loss", "rows")
    T = _transposed(transposed, idx, "loss") if transposed is not None else (None, None)
    _on_gpu("loss", features=f, idx=idx, weight=weight, rows=rows, in_ptr=T[0], in_edge=T[1])
    want = f.requires_grad and torch.is_grad_enabled()
    if want and transposed is None:
        T = transpose(idx)
    if not want:
        loss, n_edges, _ = _forward(f.detach().contiguous(), idx, weight, rows, None, False)
        return loss, n_edges
    return _SmoothLoss.apply(f, idx, weight, rows, T)


def loss(features, idx, weight=None, rows=None, transposed=None):
    """-> 0-d float32: L = (1 / N_E) sum_{counting (i,m)} w[i,m] |f[i] - f[idx[i,m]]|^2  (module docstring), with its gradient
    to `features` [P,S] (float32, 1 <= S <= 32) only.

        idx, dist2 = knn.graph(pc.get_xyz, 8)                  # once: the semantic stage has frozen geometry
        T = smooth.transpose(idx)                              # once
        ...
        loss = sem_loss + lam * smooth.loss(pc._semantics, idx, transposed=T)

    weight: float32 [P,k] (absent: 1; e.g. gaussian_weights(dist2, sigma)); no gradient goes to it.  rows: bool [P], the rows
    whose out-edges count (absent: all), e.g. a random subset redrawn every iteration -- the transpose does not depend on it.
    transposed: the pair from transpose(idx); built on the fly when absent (and a gradient is wanted).  The forward computes
    and saves the gradient when features.requires_grad and computes none otherwise; the backward is one multiply.  Two calls
    give the same bits.  No host synchronisation in forward or backward."""
    return loss_terms(features, idx, weight, rows, transposed)[0]


def gaussian_weights(dist2, sigma):
    """-> float32 [P,k]: exp(-dist2 / (2 sigma^2)) of a graph's dist2, 0 where dist2 is not finite (the +inf of a row's -1 tail).
    Torch glue on a [P,k] array, not a kernel of this package."""
    dist2 = _tensor(dist2, "gaussian_weights", "dist2", (torch.float32,))
    if dist2.dim() != 2:
        raise ValueError("smooth.gaussian_weights: dist2 must have shape (P, k)")
    sigma = float(sigma)
    if not sigma > 0 or math.isinf(sigma):
        raise ValueError("smooth.gaussian_weights: need a finite sigma > 0")
    _on_gpu("gaussian_weights", dist2=dist2)
    w = torch.exp(dist2 * (-1.0 / (2.0 * sigma * sigma)))
    return torch.where(torch.isfinite(dist2), w, torch.zeros_like(w))


def diffuse(features, idx, weight=None, fixed=None, lam=1.0, iterations=1):
    """-> a new float32 [P,S]: `iterations` Jacobi steps of

        W_i = sum_m w[i,m],  m_i = (sum_m w[i,m] f[idx[i,m]]) / W_i,  f'[i] = f[i] + lam (m_i - f[i])

    over row i's edges in slot order.  A row with fixed[i] (bool [P]), without an edge or with W_i == 0 is copied bit for bit.
    Every step reads one buffer and writes the other; `features` itself is untouched.  0 <= lam <= 1 keeps every value inside the
    range of what it averages."""
    f = _features(features, "diffuse")
    idx = _idx(idx, "diffuse", int(f.shape[0]))
    weight = _weight(weight, idx, "diffuse")
    fixed = _bytes(fixed, int(f.shape[0]), "diffuse", "fixed")
    if isinstance(iterations, bool) or not isinstance(iterations, int):
        raise TypeError("smooth.diffuse: iterations must be an int")
    if iterations < 0:
        raise ValueError("smooth.diffuse: need iterations >= 0")
    lam = float(lam)
    if math.isnan(lam):
        raise ValueError("smooth.diffuse: lam is NaN")
    _on_gpu("diffuse", features=f, idx=idx, weight=weight, fixed=fixed)
    lib = _lib.load()
    dev = f.device
    P, S, k = int(f.shape[0]), int(f.shape[1]), int(idx.shape[1])
    src = f.detach().contiguous()
    if iterations == 0:
        return src.clone()
    with torch.cuda.device(dev):
        bufs = [torch.empty_like(src), torch.empty_like(src) if iterations > 1 else None]
        for it in range(iterations):
            dst = bufs[it & 1]
            check(lib.goi_knn_diffuse(P, S, k, ptr(src), ptr(idx), ptr(weight), ptr(fixed), lam, ptr(dst), stream(dev)))
            src = dst
    return src


def complete_features(xyz, features, known, k=8, iterations=8, selection=None):
    """-> float32 [P,S]: `features` with every row that is not `known` diffused from its k nearest neighbours, the known rows
    held fixed: the continuous counterpart of knn.complete_labels.

        seen = contrib.peak_weights(cameras, pc, bg) > 0               # the Gaussians some pixel blends
        pc._semantics.data = smooth.complete_features(pc.get_xyz, pc._semantics.data, seen)

    One knn.graph(xyz, k, selection), then diffuse(features, idx, fixed=known, lam=1, iterations): after t steps a row holds an
    average of the known rows within t hops (and of the unknown rows' initial values further out, which fade as t grows).  With a
    `selection` (bool [P]) rows outside it have no neighbours and are nobody's neighbour: they are copied."""
    f = _features(features, "complete_features")
    if known is None:
        raise TypeError("smooth.complete_features: known must be a tensor")
    known = _bytes(known, int(f.shape[0]), "complete_features", "known")
    if torch.is_tensor(xyz) and xyz.dim() == 2 and xyz.shape[0] != f.shape[0]:
        raise ValueError(f"smooth.complete_features: xyz must have {int(f.shape[0])} rows, one per row of features")
    _on_gpu("complete_features", features=f, known=known)
    idx, _ = knn.graph(xyz, k, selection)
    return diffuse(f, idx, fixed=known, lam=1.0, iterations=iterations)
