"""Independent numpy restatement of the mask stage (csrc/masks.hip, goi_hyperplane_amd/masks.py) for the tests.

    dilate_reference     binary dilation by the (2r + 1)^2 square clipped at the border, from a summed-area table:
                         out[y, x] = any(m[max(0, y - r) : y + r + 1, max(0, x - r) : x + r + 1])
    confusion_reference  TP, FP, FN, TN of a prediction against a ground truth
    metrics_reference    utils/image_utils.py:59-102's three formulas from the four counts, in numpy scalars
    relevant_reference   the camera filter of gui/main.py:419-478 as written (0-d torch tensors, Python max(), the
                         removal loop), on per-camera count_nonzero values
"""
from __future__ import annotations

import numpy as np
import torch


def dilate_reference(mask: np.ndarray, r: int) -> np.ndarray:
    m = np.asarray(mask) != 0
    H, W = m.shape
    sat = np.zeros((H + 1, W + 1), np.int64)
    sat[1:, 1:] = m.astype(np.int64).cumsum(0).cumsum(1)
    y0 = np.clip(np.arange(H) - r, 0, H)[:, None]
    y1 = np.clip(np.arange(H) + r + 1, 0, H)[:, None]
    x0 = np.clip(np.arange(W) - r, 0, W)[None, :]
    x1 = np.clip(np.arange(W) + r + 1, 0, W)[None, :]
    return (sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]) > 0


def confusion_reference(pred: np.ndarray, gt: np.ndarray) -> np.ndarray:
    p, g = np.asarray(pred) != 0, np.asarray(gt) != 0
    return np.array([np.sum(p & g), np.sum(p & ~g), np.sum(~p & g), np.sum(~p & ~g)], np.int64)


def metrics_reference(counts):
    """(iou float, mpa np.float32, mp np.float32) of one view's TP, FP, FN, TN."""
    tp, fp, fn, tn = (np.int64(c) for c in counts)
    union = tp + fp + fn
    iou = float("nan") if union == 0 else float(tp) / float(max(union, 1))
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        a1 = f(tp) / f(tp + fn) if tp + fn > 0 else f(0)
        a0 = f(tn) / f(tn + fp) if tn + fp > 0 else f(0)
        p1 = f(tp) / f(tp + fp)
        p0 = f(tn) / f(tn + fn)
    return iou, f((a1 + a0) / f(2)), f((p1 + p0) / f(2))


def relevant_reference(counts, min_relative_ratio=0.1):
    """Kept camera indices of gui/main.py:419-478 given each camera's torch.count_nonzero(cos_sim)."""
    max_relative_number = 0
    relative_cameras = []
    for ind, n in enumerate(counts):
        relative_pixel_number = torch.tensor(int(n), dtype=torch.int64)
        if relative_pixel_number > 0:  # cos_sim.any(): a camera without a nonzero similarity is never appended
            max_relative_number = max(max_relative_number, relative_pixel_number)
            relative_cameras.append((ind, relative_pixel_number))
    i = 0
    while i < len(relative_cameras):
        if relative_cameras[i][1] < max_relative_number * min_relative_ratio:
            relative_cameras.remove(relative_cameras[i])
        else:
            i += 1
    return [ind for ind, _ in relative_cameras]
