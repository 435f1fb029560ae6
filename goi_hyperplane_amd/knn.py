"""`simple_knn._C.distCUDA2` over the C ABI (reference: submodules/simple-knn/ext.cpp:15-17,
spatial.cu:15-26).  points [P,3] float32 on the GPU -> [P] float32: mean squared distance to the three
nearest other points, used by scene/gaussian_model.py:147 to size the initial Gaussians."""
from __future__ import annotations

import torch

from . import _lib


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
