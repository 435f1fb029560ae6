"""Bit-packed binary masks on the device (csrc/masks.hip): the mask stage of the reference's camera sweeps.

    pack                  cos_sim > 0 and torch.count_nonzero(cos_sim)        gui/main.py:433-443
    dilate                cv2.dilate(m, np.ones((k, k)), iterations=n) >= 0.5 gui/main.py:453-459
    confusion             TP / FP / FN / TN of a prediction against a ground truth
    segmentation_metrics  calculate_iou / _mean_pixel_accuracy / _mean_precision  utils/image_utils.py:59-102

A packed buffer is int64 [V, H, ceil(W / 64)] (the bits of uint64 words): bit j of word w of row y is pixel (y, 64 w + j),
bits past W are zero.  Every function here but segmentation_metrics takes CUDA tensors only and launches asynchronously on
the current stream: none reads anything back to the host.  segmentation_metrics works on counts and runs on the host.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from ._lib import check, ptr, stream

MAX_RADIUS = 63  # GOI_MASK_MAX_RADIUS: the row pass takes its carries from the two neighbouring words only
_F32, _U8 = 0, 1  # GOI_MASK_F32, GOI_MASK_U8
_NO_CPU = "goi_hyperplane_amd.masks: tensors must live on a ROCm GPU; there is no CPU fallback"

SegMetrics = namedtuple("SegMetrics", ["iou", "mpa", "mp"])
SegMetrics.__doc__ = ("Per-view segmentation metrics (CPU tensors): iou float64 [V] (NaN for an empty union), mpa and mp "
                      "float32 [V] (mp NaN where a class is never predicted, as in the reference).")


def words(W: int) -> int:
    """64-bit words per packed row."""
    return (int(W) + 63) // 64


def radius(kernel_size: int, iterations: int) -> int:
    """The square's radius of cv2.dilate(m, np.ones((kernel_size, kernel_size)), iterations=iterations): n (k - 1) / 2.
    Raises ValueError outside k odd >= 1, iterations >= 1, radius <= 63."""
    k, n = int(kernel_size), int(iterations)
    if k != kernel_size or k < 1 or k % 2 == 0:
        raise ValueError(f"dilate: kernel_size must be an odd integer >= 1, got {kernel_size!r}")
    if n != iterations or n < 1:
        raise ValueError(f"dilate: iterations must be an integer >= 1, got {iterations!r}")
    r = n * (k - 1) // 2
    if r > MAX_RADIUS:
        raise ValueError(f"dilate: the window radius iterations * (kernel_size - 1) / 2 = {r} exceeds {MAX_RADIUS}")
    return r


def _hw(x: torch.Tensor):
    if x.dim() < 2:
        raise ValueError(f"a mask needs at least two dimensions [..., H, W], got shape {tuple(x.shape)}")
    return int(x.shape[-2]), int(x.shape[-1])


def _source(x: torch.Tensor):
    """(contiguous tensor, kernel dtype code): fp32 maps pack x > 0, bool / uint8 masks pack x != 0."""
    if not x.is_cuda:
        raise RuntimeError(_NO_CPU)
    if x.dtype == torch.float32:
        return x.contiguous(), _F32
    if x.dtype in (torch.bool, torch.uint8):
        return x.contiguous().view(torch.uint8), _U8
    raise TypeError(f"masks: expected a float32 similarity map or a bool / uint8 mask, got {x.dtype}")


def pack_into(x: torch.Tensor, packed: torch.Tensor, counts: torch.Tensor | None = None, first_view: int = 0) -> None:
    """Packs x [..., H, W] (its leading dimensions flattened to n views) into views first_view .. of `packed` (int64
    [V, H, words(W)]) and, if given, ADDS to counts (int64 [V, 2], zeroed by the caller): column 0 the pixels with x != 0
    (count_nonzero; a NaN counts), column 1 the packed bits (x > 0 for float32, x != 0 for bool / uint8).  One launch."""
    H, W = _hw(x)
    src, code = _source(x)
    n = src.numel() // (H * W) if H * W else 0
    if packed.dtype != torch.int64 or packed.dim() != 3 or tuple(packed.shape[1:]) != (H, words(W)) or not packed.is_contiguous():
        raise ValueError(f"packed must be a contiguous int64 [V, {H}, {words(W)}] tensor, got {packed.dtype} {tuple(packed.shape)}")
    if not 0 <= first_view or first_view + n > packed.shape[0]:
        raise ValueError(f"views {first_view}..{first_view + n - 1} do not fit a buffer of {packed.shape[0]}")
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (packed.shape[0], 2)
                               or not counts.is_contiguous()):
        raise ValueError(f"counts must be a contiguous int64 [{packed.shape[0]}, 2] tensor")
    if not packed.is_cuda or (counts is not None and not counts.is_cuda):
        raise RuntimeError(_NO_CPU)
    dev = src.device
    with torch.cuda.device(dev):
        check(_lib.load().goi_semantic_mask_pack(ptr(src), code, n, H, W, int(first_view), ptr(packed), ptr(counts),
                                                  stream(dev)))


def pack(x: torch.Tensor):
    """x [..., H, W] (float32 map, bool or uint8 mask) -> (packed int64 [V, H, words(W)], counts int64 [V, 2]) with V the
    product of the leading dimensions; see pack_into for the bits and the two counts."""
    H, W = _hw(x)
    if not x.is_cuda:
        raise RuntimeError(_NO_CPU)
    n = x.numel() // (H * W) if H * W else 0
    packed = torch.empty((n, H, words(W)), dtype=torch.int64, device=x.device)
    counts = torch.zeros((n, 2), dtype=torch.int64, device=x.device)
    pack_into(x, packed, counts)
    return packed, counts


def dilate_packed(packed: torch.Tensor, W: int, r: int) -> torch.Tensor:
    """A new packed buffer: every view of `packed` dilated by the (2r + 1)^2 square clipped at the border.  One launch."""
    if not packed.is_cuda:
        raise RuntimeError(_NO_CPU)
    if not 0 <= int(r) <= MAX_RADIUS:
        raise ValueError(f"dilate: radius must be in 0..{MAX_RADIUS}, got {r}")
    V, H = int(packed.shape[0]), int(packed.shape[1])
    if packed.dtype != torch.int64 or packed.dim() != 3 or packed.shape[2] != words(W):
        raise ValueError(f"packed must be int64 [V, H, {words(W)}], got {packed.dtype} {tuple(packed.shape)}")
    src = packed.contiguous()
    out = torch.empty_like(src)
    dev = src.device
    with torch.cuda.device(dev):
        check(_lib.load().goi_semantic_mask_dilate(ptr(src), ptr(out), V, H, int(W), int(r), stream(dev)))
    return out


def unpack(packed: torch.Tensor, W: int, index: torch.Tensor | None = None) -> torch.Tensor:
    """bool [K, 1, H, W]: the views `index` (int64 CUDA tensor of K view numbers; None: all V) of `packed`, unpacked in
    one launch.  An index that names no view of the buffer gives an empty mask (it is not checked on the host: no sync)."""
    if not packed.is_cuda or (index is not None and not index.is_cuda):
        raise RuntimeError(_NO_CPU)
    if packed.dtype != torch.int64 or packed.dim() != 3 or packed.shape[2] != words(W):
        raise ValueError(f"packed must be int64 [V, H, {words(W)}], got {packed.dtype} {tuple(packed.shape)}")
    H = int(packed.shape[1])
    src = packed.contiguous()
    if index is not None:
        index = index.reshape(-1).to(torch.int64).contiguous()
    K = int(packed.shape[0]) if index is None else int(index.numel())
    out = torch.empty((K, 1, H, int(W)), dtype=torch.bool, device=src.device)
    dev = src.device
    with torch.cuda.device(dev):
        check(_lib.load().goi_semantic_mask_unpack(ptr(src), int(packed.shape[0]), H, int(W), K, ptr(index), ptr(out.view(torch.uint8)),
                                                    stream(dev)))
    return out


def dilate(mask: torch.Tensor, kernel_size: int = 3, iterations: int = 5) -> torch.Tensor:
    """Binary dilation of bool / uint8 masks [..., H, W] (nonzero = set) by np.ones((kernel_size, kernel_size)) repeated
    `iterations` times, clipped at the border: the reference's cv2.dilate(m, ones((k, k)), iterations=n) >= 0.5 on a binary
    mask (gui/main.py:453-459), and scipy.ndimage.binary_dilation(m, ones((k, k)), iterations=n).  Returns bool, same
    shape.  Pack, dilate and unpack: three launches for the whole batch."""
    r = radius(kernel_size, iterations)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"dilate: expected a bool or uint8 mask, got {mask.dtype}")
    W = _hw(mask)[1]
    packed, _ = pack(mask)
    return unpack(dilate_packed(packed, W, r), W).reshape(mask.shape)


def confusion_packed(pred: torch.Tensor, gt: torch.Tensor, W: int) -> torch.Tensor:
    """int64 [V, 4] = TP, FP, FN, TN per view of two packed buffers of the same shape.  One launch."""
    if not (pred.is_cuda and gt.is_cuda):
        raise RuntimeError(_NO_CPU)
    if pred.shape != gt.shape or pred.dtype != torch.int64 or gt.dtype != torch.int64 or pred.dim() != 3 \
            or pred.shape[2] != words(W):
        raise ValueError(f"pred and gt must be int64 [V, H, {words(W)}] of one shape, got {tuple(pred.shape)}, {tuple(gt.shape)}")
    V, H = int(pred.shape[0]), int(pred.shape[1])
    p, g = pred.contiguous(), gt.contiguous()
    out = torch.empty((V, 4), dtype=torch.int64, device=p.device)
    dev = p.device
    with torch.cuda.device(dev):
        check(_lib.load().goi_semantic_mask_confusion(ptr(p), ptr(g), V, H, int(W), ptr(out), stream(dev)))
    return out


def confusion(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """int64 [V, 4] = TP, FP, FN, TN of pred against gt, both [..., H, W] of one shape (float32: x > 0; bool / uint8:
    x != 0), V the product of the leading dimensions, on the device."""
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape")
    W = _hw(pred)[1]
    return confusion_packed(pack(pred)[0], pack(gt)[0], W)


def segmentation_metrics(confusion) -> SegMetrics:
    """IoU, mPA and mP per view from TP, FP, FN, TN counts ([V, 4] int64 tensor on any device, or array-like) with the
    arithmetic of utils/image_utils.py:59-102 on same-shape masks:
        iou = float(TP) / float(max(TP + FP + FN, 1)) in float64, NaN when the union is empty;
        mpa = (a1 + a0) / 2 in float32, a1 = fp32(TP) / fp32(TP + FN) and a0 = fp32(TN) / fp32(TN + FP), each 0 when its
              class is absent from the ground truth (the counts are rounded to float32 as .float() rounds them);
        mp  = (p1 + p0) / 2 in float32, p1 = fp32(TP) / fp32(TP + FP), p0 = fp32(TN) / fp32(TN + FN), unguarded (0/0 is NaN).
    Host arithmetic on V x 4 numbers (a CUDA tensor is read back once)."""
    c = torch.as_tensor(confusion).detach().to("cpu", torch.int64).reshape(-1, 4)
    tp, fp, fn, tn = c.unbind(1)
    union = tp + fp + fn
    iou = tp.double() / union.clamp(min=1).double()
    iou = torch.where(union == 0, torch.full_like(iou, float("nan")), iou)
    gt1, gt0 = tp + fn, tn + fp
    zero = torch.zeros((), dtype=torch.float32)
    a1 = torch.where(gt1 > 0, tp.float() / gt1.float(), zero)
    a0 = torch.where(gt0 > 0, tn.float() / gt0.float(), zero)
    mpa = (a1 + a0) / 2
    mp = (tp.float() / (tp + fp).float() + tn.float() / (tn + fn).float()) / 2
    return SegMetrics(iou, mpa, mp)
