"""Float64 restatement of the photometric contract (csrc/photometric.hip, goi_hyperplane_amd.photometric), used by the
CPU and GPU tests.

ssim64 is utils/loss_utils._ssim evaluated in float64 with the reference's fp32 1-D window (loss_utils.gaussian(11, 1.5):
exp in double, rounded to fp32, normalised by its fp32 sum) and its exact outer product as the 11x11 window.  The
reference rounds that product to fp32 (create_window); that rounding is part of its fp32 error, like any other.  ssim_grad_np is the backward the kernel implements, derived
by hand and written in numpy:
    dS/dx = w * P_mu1 + 2 x (w * P_xx) + y (w * P_xy)      (w * = the zero-padded 11x11 window filter)
with P_mu1 = dS/dmu1, P_xx = dS/dE[x^2], P_xy = dS/dE[xy] per pixel, and the mirrored formula for y."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_1d() -> torch.Tensor:
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return g / g.sum()


def window_2d() -> torch.Tensor:
    """the reference's fp32 11x11 window (create_window)"""
    g = window_1d().unsqueeze(1)
    return g.mm(g.t()).float()


def window_2d64() -> torch.Tensor:
    """the exact outer product of the fp32 1-D window, in float64"""
    g = window_1d().double().unsqueeze(1)
    return g.mm(g.t())


def _as4(t):
    t = torch.as_tensor(t)
    return t.unsqueeze(0) if t.dim() == 3 else t


def ssim_map64(x, y):
    """[N, C, H, W] float64 SSIM map of loss_utils._ssim"""
    x, y = _as4(x).double(), _as4(y).double()
    C = x.shape[1]
    w = window_2d64().expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11 = conv(x * x) - mu1_sq
    s22 = conv(y * y) - mu2_sq
    s12 = conv(x * y) - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2))


def ssim64(x, y, size_average=True):
    m = ssim_map64(x, y)
    return m.mean() if size_average else m.mean(dim=(1, 2, 3))


def l1_64(x, y):
    return (torch.as_tensor(x).double() - torch.as_tensor(y).double()).abs().mean()


def psnr64(x, y):
    """image_utils.psnr in float64: per row of x.view(x.shape[0], -1), [rows, 1]"""
    x, y = torch.as_tensor(x).double(), torch.as_tensor(y).double()
    mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def loss64(x, y, lam=0.2):
    return (1.0 - lam) * l1_64(x, y) + lam * (1.0 - ssim64(x, y))


def autograd64(fn, x, y):
    """(value, d fn / dx, d fn / dy) in float64 by autograd"""
    x = torch.as_tensor(x).double().clone().requires_grad_(True)
    y = torch.as_tensor(y).double().clone().requires_grad_(True)
    v = fn(x, y)
    gx, gy = torch.autograd.grad(v.sum(), (x, y))
    return v.detach(), gx, gy


def _filter_np(a, w2):
    """zero-padded 11x11 window filter (correlation; the window is symmetric) of every [H, W] plane of a [..., H, W] array"""
    H, W = a.shape[-2:]
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(5, 5), (5, 5)])
    return sum(w2[i, j] * p[..., i:i + H, j:j + W] for i in range(11) for j in range(11))


def ssim_grad_np(x, y, size_average=True):
    """d mean-SSIM / dx and / dy of [N, C, H, W] float64 arrays by the hand-derived formula (per-image means when not
    size_average: the gradient of their sum)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w2 = window_2d64().numpy()
    f = lambda t: _filter_np(t, w2)  # noqa: E731
    mu1, mu2, exx, eyy, exy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    A1 = 2 * mu1 * mu2 + C1
    A2 = 2 * (exy - mu1 * mu2) + C2
    B1 = mu1 ** 2 + mu2 ** 2 + C1
    B2 = (exx - mu1 ** 2) + (eyy - mu2 ** 2) + C2
    S = A1 * A2 / (B1 * B2)
    inv = 1.0 / (B1 * B2)
    p_mu1 = 2 * inv * (mu2 * (A2 - A1) - mu1 * S * (B2 - B1))
    p_mu2 = 2 * inv * (mu1 * (A2 - A1) - mu2 * S * (B2 - B1))
    p_xx = -S / B2
    p_xy = 2 * A1 * inv
    fxx, fxy = f(p_xx), f(p_xy)
    gx = f(p_mu1) + 2 * x * fxx + y * fxy
    gy = f(p_mu2) + 2 * y * fxx + x * fxy
    M = x.size if size_average else x[0].size
    return gx / M, gy / M
