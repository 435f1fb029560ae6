"""Nearest neighbours of point sets on the GPU (csrc/knn.hip over the C ABI).

    distCUDA2(points)                                   -> float32 [P]: `simple_knn._C.distCUDA2`
    graph(points, k, selection=None)                    -> (idx int32 [P,k], dist2 float32 [P,k]): the k nearest OTHER points
    query(queries, refs, k, query_mask=None, ref_mask=None) -> (idx int32 [Pq,k], dist2 float32 [Pq,k])
    majority_labels(idx, labels, dist2=None, max_dist2=None) -> (label int64 [Pq], count int32 [Pq])
    complete_labels(xyz, labels, k=8, max_dist2=None, selection=None) -> int64 [P]
    mean_distance(dist2)                                -> float32 [P]
    statistical_outliers(points, k=16, ratio=2.0, selection=None) -> bool [P]

distCUDA2 (reference: submodules/simple-knn/ext.cpp:15-17, spatial.cu:15-26): points [P,3] float32 on the GPU -> [P] float32,
the mean squared distance to the three nearest other points, used by scene/gaussian_model.py:147 to size the initial Gaussians.

THE GRAPH (goi_knn_graph; the reference has no counterpart).  With
dist2(i, j) = fmaf(dz, dz, fmaf(dx, dx, dy * dy)), d = refs[j] - queries[i] in fp32, row i holds the k smallest (dist2, j) pairs
in ascending lexicographic order: ties in distance go to the lower id.  Exact, the same bits every run and for any order of the
input; ids are the caller's.  A masked-out reference is never a neighbour; the row of a masked-out query, and the tail of a row
with fewer than k references, is idx = -1, dist2 = +inf.  1 <= k <= 16.  Nothing is gathered, nothing is read back: the masks
go to the kernels as they are and the kept counts stay on the device.  fp32 tensors on a ROCm GPU only; there is no CPU
fallback.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import check, ptr, stream

_NO_CPU = "goi_hyperplane_amd.knn: tensors must live on a ROCm GPU; there is no CPU fallback"
K_MAX = 16  # goi_knn_graph: 1 <= k <= 16


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    if points.dim() >= 1 and points.size(0) >= 2 ** 30:  # (the radix sort of the Morton codes is exact below 2^30 keys)
        raise RuntimeError("distCUDA2: at most 2^30 - 1 points")
    if not points.is_cuda:
        raise RuntimeError("distCUDA2: points must live on a ROCm GPU (cuda device); there is no CPU fallback")
    if points.dtype != torch.float32:
        raise TypeError(f"distCUDA2: points must be float32, got {points.dtype}")  # ref: .data<float>() throws
    P = int(points.size(0))
    dev = points.device
    pts = points.contiguous()
    with torch.cuda.device(dev):
        means = torch.zeros((P,), dtype=torch.float32, device=dev)  # spatial.cu:21: torch::full({P}, 0.0)
        if P == 0:
            return means
        if pts.numel() != 3 * P:
            raise RuntimeError("distCUDA2: points must have shape (P, 3)")
        ws = torch.empty(lib.goi_knn_workspace_bytes(P), dtype=torch.uint8, device=dev)
        _lib.check(lib.goi_knn_dist2(P, _lib.ptr(pts), _lib.ptr(means), _lib.ptr(ws), _lib.stream(dev)))
    return means


def _points(t, who, what):
    """[P,3] float32 on the device, contiguous (a contiguous input is passed as it is: graph() relies on the same pointer)"""
    if not torch.is_tensor(t):
        raise TypeError(f"knn.{who}: {what} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(_NO_CPU)
    if t.dtype != torch.float32:
        raise TypeError(f"knn.{who}: {what} must be float32, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"knn.{who}: {what} must have shape (P, 3)")
    if t.shape[0] >= 2 ** 30:
        raise ValueError(f"knn.{who}: at most 2^30 - 1 points")
    return t.detach().contiguous()


def _mask(m, P, dev, who, what):
    """bool (or uint8) [P] on the device -> contiguous uint8 (a view of a contiguous bool: no copy); None stays None"""
    if m is None:
        return None
    if not torch.is_tensor(m):
        raise TypeError(f"knn.{who}: {what} must be a tensor")
    if not m.is_cuda:
        raise RuntimeError(_NO_CPU)
    if m.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"knn.{who}: {what} must be bool or uint8, got {m.dtype}")
    if tuple(m.shape) != (P,):
        raise ValueError(f"knn.{who}: {what} must have shape ({P},)")
    if m.device != dev:
        raise ValueError(f"knn.{who}: {what} is on {m.device}, expected {dev}")
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _k(k, who):
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"knn.{who}: k must be an int")
    if not 1 <= k <= K_MAX:
        raise ValueError(f"knn.{who}: need 1 <= k <= {K_MAX}")
    return k


def _graph(q, qm, r, rm, k, exclude_self):
    lib = _lib.load()
    dev = q.device
    Pq, Pr = int(q.shape[0]), int(r.shape[0])
    with torch.cuda.device(dev):
        idx = torch.empty((Pq, k), dtype=torch.int32, device=dev)
        dist2 = torch.empty((Pq, k), dtype=torch.float32, device=dev)
        if Pq:
            ws = _lib.workspace(lib.goi_knn_graph_workspace_bytes(Pq, Pr), dev)
            check(lib.goi_knn_graph(Pq, ptr(q), ptr(qm), Pr, ptr(r), ptr(rm), k, int(exclude_self), ptr(idx), ptr(dist2), ptr(ws),
                                    stream(dev)))
    return idx, dist2


def graph(points, k, selection=None):
    """-> (idx int32 [P,k], dist2 float32 [P,k]): the k nearest OTHER points of every point (the point itself is excluded, a
    coincident one is not).  selection: a bool [P] mask for both sides -- only selected points are queries, only selected points
    are neighbours; an unselected row is -1 / +inf.  Asynchronous, no read-back."""
    k = _k(k, "graph")
    pts = _points(points, "graph", "points")
    keep = _mask(selection, int(pts.shape[0]), pts.device, "graph", "selection")
    return _graph(pts, keep, pts, keep, k, True)


def query(queries, refs, k, query_mask=None, ref_mask=None):
    """-> (idx int32 [Pq,k], dist2 float32 [Pq,k]): the k nearest references of every query, ids into `refs`.  Nothing is
    excluded: a reference coincident with the query counts, with distance 0.  query_mask bool [Pq] / ref_mask bool [Pr]: who
    asks and who may be found.  The queries may lie anywhere, outside the references' bounds included."""
    k = _k(k, "query")
    q = _points(queries, "query", "queries")
    r = _points(refs, "query", "refs")
    if r.device != q.device:
        raise ValueError(f"knn.query: refs is on {r.device}, expected {q.device}")
    qm = _mask(query_mask, int(q.shape[0]), q.device, "query", "query_mask")
    rm = _mask(ref_mask, int(r.shape[0]), q.device, "query", "ref_mask")
    return _graph(q, qm, r, rm, k, False)


def majority_labels(idx, labels, dist2=None, max_dist2=None):
    """-> (label int64 [Pq], count int32 [Pq]) of a graph's rows: the label most of a row's neighbours carry, the LOWEST label
    among equals (contrib.assign's rule), and how many carry it.  A neighbour counts with idx >= 0, labels[idx] >= 0 and, with
    max_dist2 (which needs dist2), dist2 <= max_dist2.  A row without one gets -1 and 0.  labels: int64 [Pr], any values (they
    are compared, not binned)."""
    if not torch.is_tensor(idx) or not torch.is_tensor(labels):
        raise TypeError("knn.majority_labels: idx and labels must be tensors")
    if not idx.is_cuda or not labels.is_cuda or (dist2 is not None and not dist2.is_cuda):
        raise RuntimeError(_NO_CPU)
    for name, t in (("labels", labels), ("dist2", dist2)):
        if t is not None and t.device != idx.device:
            raise ValueError(f"knn.majority_labels: {name} is on {t.device}, expected {idx.device}")
    if idx.dtype != torch.int32:
        raise TypeError(f"knn.majority_labels: idx must be int32, got {idx.dtype}")
    if labels.dtype != torch.int64:
        raise TypeError(f"knn.majority_labels: labels must be int64, got {labels.dtype}")
    if idx.dim() != 2 or idx.shape[1] < 1 or labels.dim() != 1:
        raise ValueError("knn.majority_labels: idx must have shape (Pq, k) with k >= 1 and labels shape (Pr,)")
    if max_dist2 is not None and dist2 is None:
        raise ValueError("knn.majority_labels: max_dist2 needs dist2")
    if dist2 is not None:
        if dist2.dtype != torch.float32:
            raise TypeError(f"knn.majority_labels: dist2 must be float32, got {dist2.dtype}")
        if dist2.shape != idx.shape:
            raise ValueError("knn.majority_labels: dist2 must have idx's shape")
        dist2 = dist2.contiguous()
    cut = math.inf if max_dist2 is None else float(max_dist2)
    if math.isnan(cut):
        raise ValueError("knn.majority_labels: max_dist2 is NaN")
    lib = _lib.load()
    dev = idx.device
    Pq, k = int(idx.shape[0]), int(idx.shape[1])
    idx, labels = idx.contiguous(), labels.contiguous()
    with torch.cuda.device(dev):
        label = torch.empty((Pq,), dtype=torch.int64, device=dev)
        count = torch.empty((Pq,), dtype=torch.int32, device=dev)
        check(lib.goi_knn_majority(Pq, k, ptr(idx), ptr(dist2), cut, int(labels.shape[0]), ptr(labels), ptr(label), ptr(count),
                                   stream(dev)))
    return label, count


def complete_labels(xyz, labels, k=8, max_dist2=None, selection=None):
    """-> int64 [P]: `labels` with every unlabelled (-1) Gaussian given the majority label of its k nearest LABELLED Gaussians.

        votes = contrib.votes(cameras, pc, bg, label_maps, K)      # exact blend weights per (Gaussian, class)
        labels, _ = contrib.assign(votes)                          # -1 for every Gaussian no pixel blends
        labels = knn.complete_labels(pc.get_xyz, labels, k=8)      # ... which take their neighbours' label here

    References are the Gaussians with labels >= 0, queries those with -1, both restricted to `selection` (bool [P]) when given:
    one query() through the two masks (nothing is gathered), then majority_labels.  Labelled Gaussians keep their labels; a
    query without an admissible neighbour (none labelled, none within max_dist2, or itself outside the selection) stays -1."""
    k = _k(k, "complete_labels")
    pts = _points(xyz, "complete_labels", "xyz")
    if not torch.is_tensor(labels):
        raise TypeError("knn.complete_labels: labels must be a tensor")
    if not labels.is_cuda:
        raise RuntimeError(_NO_CPU)
    if labels.device != pts.device:
        raise ValueError(f"knn.complete_labels: labels is on {labels.device}, expected {pts.device}")
    if labels.dtype != torch.int64:
        raise TypeError(f"knn.complete_labels: labels must be int64, got {labels.dtype}")
    if tuple(labels.shape) != (int(pts.shape[0]),):
        raise ValueError(f"knn.complete_labels: labels must have shape ({int(pts.shape[0])},)")
    sel = _mask(selection, int(pts.shape[0]), pts.device, "complete_labels", "selection")
    have = labels >= 0
    ask = ~have
    if sel is not None:
        have, ask = have & (sel != 0), ask & (sel != 0)
    idx, dist2 = _graph(pts, ask.view(torch.uint8), pts, have.view(torch.uint8), k, False)
    found, _ = majority_labels(idx, labels, dist2, max_dist2)
    return torch.where(labels >= 0, labels, found)


def mean_distance(dist2):
    """float32 [P]: the mean of sqrt(dist2) over the finite entries of each row of a graph's dist2; +inf for a row with none."""
    if not torch.is_tensor(dist2):
        raise TypeError("knn.mean_distance: dist2 must be a tensor")
    if not dist2.is_cuda:
        raise RuntimeError(_NO_CPU)
    if dist2.dtype != torch.float32:
        raise TypeError(f"knn.mean_distance: dist2 must be float32, got {dist2.dtype}")
    if dist2.dim() != 2:
        raise ValueError("knn.mean_distance: dist2 must have shape (P, k)")
    finite = torch.isfinite(dist2)
    n = finite.sum(dim=1)
    total = torch.where(finite, dist2.sqrt(), 0.0).sum(dim=1)
    return torch.where(n > 0, total / n.clamp(min=1).float(), math.inf)


def statistical_outliers(points, k=16, ratio=2.0, selection=None):
    """bool [P]: True where a point's mean distance to its k nearest other points is above mu + ratio * sigma, mu and sigma
    (divisor n - 1) taken over the finite scores in float64 on the device: floaters left after a retrieval.  With `selection`
    the graph and the statistics are those of the selected points and an unselected point is never an outlier.  The
    synchronisation-free part of this function is the graph; the statistics are torch glue on [P] arrays."""
    idx, dist2 = graph(points, k, selection)
    score = mean_distance(dist2)
    finite = torch.isfinite(score)
    s = torch.where(finite, score.double(), 0.0)
    n = finite.sum().double()
    mu = s.sum() / n.clamp(min=1)
    var = torch.where(finite, (score.double() - mu) ** 2, 0.0).sum() / (n - 1).clamp(min=1)
    return finite & (score.double() > mu + float(ratio) * var.sqrt())
