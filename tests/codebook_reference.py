"""Torch restatements of the code-book initialisation contract (csrc/codebook_init.hip), used by the CPU and GPU tests.

kmeans_preperm is io.kmeans (train.py:36-56) with its permutations drawn up front, in the reference's order (the seed
permutation, then one per iteration whether or not a centre is dead), and handed in: the kernel's contract.  On the
CPU it equals io.kmeans bit for bit (tests/test_codebook_cpu.py), which is what makes the up-front draws legitimate.

unique_rows_by_keys is unique(dim=0) as the kernel computes it: each float becomes an order-preserving uint32 key
(-0 folded onto +0); rows are deduplicated and sorted lexicographically on those keys; the first pixel of each class
is the row kept."""
from __future__ import annotations

import numpy as np
import torch


def draw_perms(n: int, niter: int):
    return [torch.randperm(n) for _ in range(niter + 1)]


def kmeans_preperm(x: torch.Tensor, ncluster: int, niter: int, perms) -> torch.Tensor:
    N, D = x.size()
    x /= x.norm(dim=1, keepdim=True)
    centers = x[perms[0][:ncluster]]
    for it in range(niter):
        centers = centers / centers.norm(dim=1, keepdim=True)
        assignments = (x @ centers.T).argmax(1)
        sums = torch.zeros((ncluster, D), dtype=x.dtype, device=x.device).index_add_(0, assignments, x)
        counts = torch.bincount(assignments, minlength=ncluster).to(x.dtype)
        centers = sums / counts[:, None]
        nanix = torch.any(torch.isnan(centers), dim=1)
        ndead = int(nanix.sum().item())
        if ndead > N:
            raise RuntimeError(f"{ndead} dead centres, {N} rows")
        centers[nanix] = x[perms[it + 1][:ndead]]
    return centers


def order_keys(a: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).copy()
    u[(u << np.uint32(1)) == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unique_rows_by_keys(chw: torch.Tensor) -> torch.Tensor:
    rows = chw.permute(1, 2, 0).reshape(-1, chw.shape[0]).float().numpy()
    keys = order_keys(rows)
    _, first = np.unique(keys, axis=0, return_index=True)  # lexicographic on the keys; first occurrence of each
    return torch.from_numpy(rows[first])
