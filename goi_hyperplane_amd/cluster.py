"""Exact DBSCAN on the GPU (csrc/dbscan.hip behind goi_semantic_dbscan).

    dbscan(points, eps, min_samples, return_core=False)   CUDA float32 [n, 3] -> int64 labels [n] (+ bool core mask)
    DBSCAN(eps=0.5, min_samples=5)                        sklearn.cluster.DBSCAN's minimal surface: fit, fit_predict,
                                                          labels_, core_sample_indices_

The labels equal sklearn.cluster.DBSCAN(eps, min_samples).fit(X).labels_ with the neighbour test evaluated in fp32 as
d2 = fma(dz, dz, fma(dy, dy, dx * dx)) <= eps * eps (include/goi_raster.h, csrc/dbscan.hip).  gui/main.py:32 switches by
importing DBSCAN from here instead of sklearn.cluster; numpy input gives numpy output, as the reference's call expects.
There is no CPU path: a CPU tensor is an error, and a numpy array is copied to the current GPU and back.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

FLAG_NONFINITE, FLAG_SORT, FLAG_RANGE, FLAG_GRID, FLAG_UNION = 1, 2, 4, 8, 16  # include/goi_raster.h DBSCAN_FLAG_*

_NO_CPU = "goi_hyperplane_amd.cluster: tensors must live on a ROCm GPU; there is no CPU fallback"


def _check_params(eps, min_samples):
    """sklearn 1.7's parameter validation of DBSCAN (the same messages; ValueError)."""
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not 0.0 < float(eps) < float("inf"):
        raise ValueError(f"The 'eps' parameter of DBSCAN must be a float in the range (0.0, inf). Got {eps!r} instead.")
    if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or int(min_samples) < 1:
        raise ValueError(f"The 'min_samples' parameter of DBSCAN must be an int in the range [1, inf). "
                         f"Got {min_samples!r} instead.")


def _flag_error(flags: int, points: torch.Tensor) -> Exception:
    if flags & FLAG_NONFINITE:
        if bool(torch.isnan(points).any()):
            return ValueError("Input X contains NaN.")
        return ValueError("Input X contains infinity or a value too large for dtype('float32').")
    if flags & FLAG_RANGE:
        return ValueError("dbscan: the point set's extent needs more than 2^21 grid cells of side eps/sqrt(3) on an axis, or "
                          "eps is outside [2^-40, 2^40]; the exact grid does not cover it")
    if flags & FLAG_SORT:
        return RuntimeError("dbscan: a radix-sort look-back ran out of its budget (the device is wedged or preempted)")
    return RuntimeError(f"dbscan: internal consistency check failed (flags {flags:#x})")


@torch.no_grad()
def dbscan(points: torch.Tensor, eps: float, min_samples: int, return_core: bool = False):
    """Labels (int64 [n], -1 = noise) of sklearn's DBSCAN on a CUDA float32 [n, 3] tensor, and the bool core mask [n] when
    return_core.  Asynchronous HIP work on the current stream and ONE synchronisation, to read the cluster count and the
    device flag word (NaN / inf input raises ValueError as sklearn does).  The cluster count is dbscan.last_n_clusters."""
    _check_params(eps, min_samples)
    if not torch.is_tensor(points):
        raise TypeError("dbscan: points must be a torch tensor (DBSCAN.fit also takes numpy arrays)")
    if points.dtype != torch.float32:
        raise TypeError(f"dbscan: points must be float32, got {points.dtype}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"dbscan: points must be [n, 3], got {tuple(points.shape)}")
    n = int(points.shape[0])
    if n >= 2 ** 30:  # (the radix sort of the cell keys is exact below 2^30 keys: csrc/common.h)
        raise ValueError("dbscan: at most 2^30 - 1 points")
    if not points.is_cuda:
        raise RuntimeError(_NO_CPU)
    dev = points.device
    pts = points.contiguous()
    lib = _lib.load()
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    core = torch.empty(n, dtype=torch.uint8, device=dev) if return_core else None
    result = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.goi_semantic_dbscan_workspace_bytes(n)), 1), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(lib.goi_semantic_dbscan(n, p(pts), float(eps), int(min_samples), p(labels), p(core), p(result), p(ws),
                                           _lib.stream(dev)), ValueError)
    n_clusters, flags = (int(v) for v in result.cpu())  # the one synchronisation
    if flags:
        raise _flag_error(flags, pts)
    dbscan.last_n_clusters = n_clusters
    out = labels.long()
    return (out, core.bool()) if return_core else out


dbscan.last_n_clusters = 0


class DBSCAN:
    """sklearn.cluster.DBSCAN(eps, min_samples) for 3-d float32 points, computed by dbscan().  fit(X) takes a numpy array
    or a CUDA tensor and sets labels_ and core_sample_indices_ of the same kind (numpy int64, or int64 tensors on X's
    device); fit_predict(X) returns labels_.  Other metrics, sample_weight, algorithm and leaf_size are not offered."""

    def __init__(self, eps: float = 0.5, min_samples: int = 5):
        self.eps = eps
        self.min_samples = min_samples

    def fit(self, X, y=None):
        _check_params(self.eps, self.min_samples)
        if isinstance(X, np.ndarray):
            if X.dtype != np.float32:
                raise TypeError(f"DBSCAN: X must be float32, got {X.dtype}")
            labels, core = dbscan(torch.from_numpy(np.ascontiguousarray(X)).cuda(), self.eps, self.min_samples, return_core=True)
            self.labels_ = labels.cpu().numpy()
            self.core_sample_indices_ = torch.nonzero(core).reshape(-1).cpu().numpy()
        elif torch.is_tensor(X):
            if X.dtype != torch.float32:
                raise TypeError(f"DBSCAN: X must be float32, got {X.dtype}")
            labels, core = dbscan(X, self.eps, self.min_samples, return_core=True)
            self.labels_ = labels
            self.core_sample_indices_ = torch.nonzero(core).reshape(-1)
        else:
            raise TypeError(f"DBSCAN: X must be a numpy array or a CUDA tensor, got {type(X).__name__}")
        self.n_clusters_ = dbscan.last_n_clusters
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
