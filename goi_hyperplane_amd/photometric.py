"""Photometric loss and image metrics of 3DGS training on the device (csrc/photometric.hip).

Drop-ins for the reference's image-space arithmetic, each one fused HIP forward (and one HIP backward):
    ssim(img1, img2, window_size=11, size_average=True)   utils/loss_utils.ssim
    l1_loss(a, b)                                          utils/loss_utils.l1_loss
    psnr(a, b)                                             utils/image_utils.psnr
    photometric_loss(image, gt, lambda_dssim=0.2)          train.py:137-140, (1 - lambda) L1 + lambda (1 - SSIM)
    image_metrics(renders, gts)                            per-image SSIM / PSNR / L1 of training_report and metrics.py

Images are [C, H, W] or [N, C, H, W] float32 on a ROCm GPU.  Results stay on the device and no call synchronises the
host.  Sums are formed in a fixed order, so two calls give the same bits.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from ._lib import check, ptr, stream

_NO_CPU = "goi_hyperplane_amd.photometric: tensors must live on a ROCm GPU; there is no CPU fallback"

_GRAD1, _GRAD2, _PER_IMAGE, _SSIM_ONLY = 1, 2, 4, 8  # GOI_PHOTOMETRIC_* of include/goi_raster.h
WINDOW_SIZE = 11

ImageMetrics = namedtuple("ImageMetrics", ["ssim", "psnr", "l1"])
PhotometricTerms = namedtuple("PhotometricTerms", ["l1", "ssim"])


def _check(img1, img2, fn, window_size=WINDOW_SIZE):
    """[N, C, H, W] contiguous views of the two images; raises as the rest of the package does."""
    if int(window_size) != WINDOW_SIZE:
        raise ValueError(f"{fn}: window_size {window_size} is not supported (only 11, the size every reference caller uses)")
    for name, t in (("img1", img1), ("img2", img2)):
        if not torch.is_tensor(t):
            raise TypeError(f"{fn}: {name} must be a tensor")
        if t.dim() not in (3, 4):
            raise ValueError(f"{fn}: {name} must be [C, H, W] or [N, C, H, W], got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{fn}: {name} must be torch.float32, got {t.dtype}")
    if img1.shape != img2.shape:
        raise ValueError(f"{fn}: shapes differ: {tuple(img1.shape)} vs {tuple(img2.shape)}")
    if img1.numel() == 0:
        raise ValueError(f"{fn}: empty images")
    if not img1.is_cuda or not img2.is_cuda:
        raise RuntimeError(_NO_CPU)
    if img1.device != img2.device:
        raise ValueError(f"{fn}: img2 is on {img2.device}, expected {img1.device}")
    a, b = img1.contiguous(), img2.contiguous()
    if a.dim() == 3:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    return a, b


def _forward(a, b, lam, flags, per_image):
    """One fused forward over [N, C, H, W] a, b: (out [3] = loss, L1, SSIM; per-image [3, N] = SSIM, L1, PSNR or None;
    the workspace the backward reads)."""
    lib = _lib.load()
    N, Ch, H, W = (int(s) for s in a.shape)
    dev = a.device
    nbytes = int(lib.goi_raster_photometric_workspace_bytes(N, Ch, H, W, flags))
    if nbytes == 0:
        raise ValueError(f"photometric: shape {tuple(a.shape)} is out of range")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    imgs = torch.empty(3, N, dtype=torch.float32, device=dev) if per_image else None
    with torch.cuda.device(dev):
        check(lib.goi_raster_photometric_forward(ptr(a), ptr(b), N, Ch, H, W, WINDOW_SIZE, float(lam), flags, ptr(out), ptr(imgs), ptr(ws),
                                                 stream(dev)), ValueError)
    return out, imgs, ws


def _backward(a, b, lam, flags, grad_out, ws, need1, need2):
    lib = _lib.load()
    N, Ch, H, W = (int(s) for s in a.shape)
    dev = a.device
    g = grad_out.detach().to(device=dev, dtype=torch.float32).contiguous()
    g1 = torch.empty_like(a) if need1 else None
    g2 = torch.empty_like(b) if need2 else None
    flags |= (_GRAD1 if need1 else 0) | (_GRAD2 if need2 else 0)
    with torch.cuda.device(dev):
        check(lib.goi_raster_photometric_backward(ptr(a), ptr(b), N, Ch, H, W, WINDOW_SIZE, float(lam), flags, ptr(g), ptr(ws), ptr(g1),
                                                  ptr(g2), stream(dev)), ValueError)
    return g1, g2


def _grad_flags(ctx):
    return (_GRAD1 if ctx.needs_input_grad[0] else 0) | (_GRAD2 if ctx.needs_input_grad[1] else 0)


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, size_average):
        a, b = _check(img1, img2, "ssim")
        flags = _grad_flags(ctx)
        out, imgs, ws = _forward(a, b, 0.0, flags, not size_average)
        ctx.shape, ctx.size_average = img1.shape, size_average
        ctx.ws = ws
        ctx.save_for_backward(a, b)
        return out[2] if size_average else imgs[0]

    @staticmethod
    def backward(ctx, grad):
        a, b = ctx.saved_tensors
        flags = _SSIM_ONLY | (0 if ctx.size_average else _PER_IMAGE)
        g1, g2 = _backward(a, b, 0.0, flags, grad, ctx.ws, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (None if g1 is None else g1.view(ctx.shape)), (None if g2 is None else g2.view(ctx.shape)), None


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lam):
        a, b = _check(image, gt, "photometric_loss")
        out, _, ws = _forward(a, b, lam, _grad_flags(ctx), False)
        ctx.shape, ctx.lam, ctx.ws = image.shape, lam, ws
        ctx.save_for_backward(a, b)
        l1, s = out[1].clone(), out[2].clone()
        ctx.mark_non_differentiable(l1, s)
        return out[0], l1, s

    @staticmethod
    def backward(ctx, grad, _g_l1, _g_ssim):
        a, b = ctx.saved_tensors
        g1, g2 = _backward(a, b, ctx.lam, 0, grad, ctx.ws, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (None if g1 is None else g1.view(ctx.shape)), (None if g2 is None else g2.view(ctx.shape)), None


def ssim(img1, img2, window_size: int = 11, size_average: bool = True):
    """loss_utils.ssim: the mean of the SSIM map (size_average) or, for [N, C, H, W] input, its mean per image [N].
    Differentiable in both images."""
    if int(window_size) != WINDOW_SIZE:
        _check(img1, img2, "ssim", window_size)
    if not size_average and torch.is_tensor(img1) and img1.dim() == 3:
        # the reference's ssim_map.mean(1).mean(1).mean(1) has no third dimension to reduce for a [C, H, W] image
        raise ValueError("ssim: size_average=False needs [N, C, H, W] input (the reference raises for [C, H, W])")
    return _SSIM.apply(img1, img2, bool(size_average))


def photometric_loss(image, gt, lambda_dssim: float = 0.2):
    """train.py:137-140: loss = (1 - lambda) * l1_loss(image, gt) + lambda * (1 - ssim(image, gt)), from one fused forward;
    its backward is one kernel.  Returns (loss, terms) with terms.l1 and terms.ssim the detached scalars, on the device."""
    loss, l1, s = _Loss.apply(image, gt, float(lambda_dssim))
    return loss, PhotometricTerms(l1, s)


def l1_loss(network_output, gt):
    """loss_utils.l1_loss: mean |network_output - gt| (a scalar); differentiable in both."""
    return _Loss.apply(network_output, gt, 0.0)[0]


@torch.no_grad()
def psnr(img1, img2):
    """image_utils.psnr: 20 log10(1 / sqrt(mse)) per row of img1.view(img1.shape[0], -1), as [rows, 1]: per image of an
    [N, C, H, W] batch, per channel of a [C, H, W] image (as the reference's view makes it)."""
    a, b = _check(img1, img2, "psnr")
    if img1.dim() == 3:
        a, b = a.view(-1, 1, *a.shape[2:]), b.view(-1, 1, *b.shape[2:])
    _, imgs, _ = _forward(a, b, 0.0, 0, True)
    return imgs[2].unsqueeze(1)


@torch.no_grad()
def image_metrics(renders, gts) -> ImageMetrics:
    """Per-image SSIM, PSNR and L1 ([N] each; [1] for a [C, H, W] image) of a batch from one forward, no backward: the
    quantities metrics.py (ssim, psnr per view) and training_report (l1_loss, psnr per view) compute."""
    a, b = _check(renders, gts, "image_metrics")
    _, imgs, _ = _forward(a, b, 0.0, 0, True)
    return ImageMetrics(imgs[0], imgs[2], imgs[1])
