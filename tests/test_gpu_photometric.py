"""The photometric loss and image metrics of csrc/photometric.hip on the GPU (goi_hyperplane_amd.photometric).

Every value and gradient is held against the float64 restatement (tests/photometric_reference.py) with the budget the
reference's own fp32 arithmetic sets: max |ours - f64| <= 2 max |torch fp32 - f64| + 1e-6 per tensor, torch fp32 being
loss_utils' F.conv2d restatement on the CPU (the pinned reference values for the golden cases).  Shapes cover 1x1,
3x4x6, one pixel either side of the 32-pixel tile edges, 800x528 and 1600x1056, batches of 4 with per-image means,
C = 1 and 3, lambda = 0, 0.2 and 1, a constant image and exactly equal images.  Two calls give the same bits, nothing
synchronises the host, and render -> photometric_loss -> backward gives the Gaussian gradients of the reference's
F.conv2d loss."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import photometric
from tests import photometric_reference as pr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_photometric_pins.npz")
DEV = torch.device("cuda")


def ssim32(x, y, size_average=True):
    """loss_utils._ssim in fp32 on the CPU (the reference's arithmetic)"""
    x4, y4 = (t.unsqueeze(0) if t.dim() == 3 else t for t in (x, y))
    C = x4.shape[1]
    w = pr.window_2d().expand(C, 1, 11, 11).contiguous()
    conv = lambda t: torch.nn.functional.conv2d(t, w, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = conv(x4), conv(y4)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11, s22, s12 = conv(x4 * x4) - mu1_sq, conv(y4 * y4) - mu2_sq, conv(x4 * y4) - mu1_mu2
    m = ((2 * mu1_mu2 + pr.C1) * (2 * s12 + pr.C2)) / ((mu1_sq + mu2_sq + pr.C1) * (s11 + s22 + pr.C2))
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def loss32(x, y, lam):
    return (1.0 - lam) * torch.abs(x - y).mean() + lam * (1.0 - ssim32(x, y))


def autograd32(fn, x, y):
    x = x.clone().requires_grad_(True)
    y = y.clone().requires_grad_(True)
    v = fn(x, y)
    gx, gy = torch.autograd.grad(v.sum(), (x, y))
    return v.detach(), gx, gy


def within(ours, t32, t64, what):
    ours = torch.as_tensor(ours).detach().double().cpu()
    t32, t64 = torch.as_tensor(t32).double().cpu(), torch.as_tensor(t64).double().cpu()
    assert ours.shape == t64.shape, what
    inf = torch.isinf(t64)
    assert torch.equal(torch.isinf(ours), inf), f"{what}: infinities differ"
    ours, t32, t64 = ours[~inf], t32[~inf], t64[~inf]
    if ours.numel() == 0:
        return
    e_ours = float((ours - t64).abs().max())
    e_ref = float((t32 - t64).abs().max())
    assert e_ours <= 2 * e_ref + 1e-6, f"{what}: |ours - f64| = {e_ours:.3e} > 2 x {e_ref:.3e} + 1e-6"


def pair(shape, seed, kind="random"):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    y = (x + 0.15 * torch.randn(shape, generator=g)).clamp(0, 1)
    if kind == "const":
        x = torch.full(shape, 0.5)
    elif kind == "equal":
        y = x.clone()
    elif kind == "patches":  # x == y on a block
        sl = (Ellipsis, slice(0, shape[-2] // 2), slice(0, shape[-1] // 3))
        y[sl] = x[sl]
    return x, y


def check_loss(x, y, lam):
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    loss, terms = photometric.photometric_loss(xg, yg, lam)
    loss.backward()
    v64, gx64, gy64 = pr.autograd64(lambda a, b: pr.loss64(a, b, lam), x, y)
    v32, gx32, gy32 = autograd32(lambda a, b: loss32(a, b, lam), x, y)
    within(loss, v32, v64, "loss")
    within(xg.grad, gx32, gx64, "d loss / d image")
    within(yg.grad, gy32, gy64, "d loss / d gt")
    within(terms.l1, torch.abs(x - y).mean(), pr.l1_64(x, y), "l1")
    within(terms.ssim, ssim32(x, y), pr.ssim64(x, y), "ssim")


def check_ssim(x, y, size_average=True):
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    s = photometric.ssim(xg, yg, size_average=size_average)
    s.sum().backward()
    v64, gx64, gy64 = pr.autograd64(lambda a, b: pr.ssim64(a, b, size_average), x, y)
    v32, gx32, gy32 = autograd32(lambda a, b: ssim32(a, b, size_average), x, y)
    within(s, v32, v64, "ssim")
    within(xg.grad, gx32, gx64, "d ssim / d img1")
    within(yg.grad, gy32, gy64, "d ssim / d img2")


def check_metrics(x, y):
    x4, y4 = (t.unsqueeze(0) if t.dim() == 3 else t for t in (x, y))
    m = photometric.image_metrics(x.to(DEV), y.to(DEV))
    within(m.ssim, ssim32(x4, y4, False), pr.ssim64(x4, y4, False), "per-image ssim")
    within(m.l1, torch.abs(x4 - y4).mean(dim=(1, 2, 3)), (x4.double() - y4.double()).abs().mean(dim=(1, 2, 3)), "per-image l1")
    p = photometric.psnr(x.to(DEV), y.to(DEV))
    mse32 = ((x - y) ** 2).view(x.shape[0], -1).mean(1, keepdim=True)
    within(p, 20 * torch.log10(1.0 / torch.sqrt(mse32)), pr.psnr64(x, y), "psnr")
    assert torch.equal(m.psnr.cpu(), photometric.psnr(x4.to(DEV), y4.to(DEV)).view(-1).cpu())
    within(photometric.l1_loss(x.to(DEV), y.to(DEV)), torch.abs(x - y).mean(), pr.l1_64(x, y), "l1_loss")


def test_golden_pins():
    z = np.load(GOLD)
    lam = float(z["lambda_dssim"])
    for name in ("hw", "batch", "tiny", "const", "equal"):
        x, y = (torch.from_numpy(z[f"{name}_{k}"]).float() / 255 for k in ("x", "y"))
        xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
        loss, terms = photometric.photometric_loss(xg, yg, lam)
        loss.backward()
        _, gx64, gy64 = pr.autograd64(lambda a, b: pr.loss64(a, b, lam), x, y)
        within(loss, z[f"{name}_loss"], pr.loss64(x, y, lam), f"{name} loss")
        within(terms.l1, z[f"{name}_l1"], pr.l1_64(x, y), f"{name} l1")
        within(terms.ssim, z[f"{name}_ssim"], pr.ssim64(x, y), f"{name} ssim")
        within(xg.grad, z[f"{name}_loss_gx"], gx64, f"{name} d loss / dx")
        within(yg.grad, z[f"{name}_loss_gy"], gy64, f"{name} d loss / dy")
        p64 = pr.psnr64(x, y)
        p = photometric.psnr(x.to(DEV), y.to(DEV)).cpu()
        pin = torch.from_numpy(z[f"{name}_psnr"])
        assert p.shape == pin.shape and torch.equal(torch.isinf(p), torch.isinf(pin))
        fin = torch.isfinite(p64)
        within(p[fin], pin[fin], p64[fin], f"{name} psnr")
        if name == "batch":
            s = photometric.ssim(x.to(DEV), y.to(DEV), size_average=False)
            within(s, z["batch_ssim_per_image"], pr.ssim64(x, y, False), "batch per-image ssim")
        else:
            xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
            photometric.ssim(xg, yg).backward()
            _, sx64, sy64 = pr.autograd64(pr.ssim64, x, y)
            within(xg.grad, z[f"{name}_ssim_gx"], sx64, f"{name} d ssim / dx")
            within(yg.grad, z[f"{name}_ssim_gy"], sy64, f"{name} d ssim / dy")


EDGE_SHAPES = [(1, 1, 1), (3, 4, 6), (1, 31, 33), (1, 33, 31), (3, 32, 32), (1, 63, 65), (3, 65, 64), (1, 5, 97), (3, 96, 2)]


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_small_and_tile_edge_shapes(shape):
    x, y = pair(shape, seed=sum(shape), kind="patches")
    check_loss(x, y, 0.2)
    check_ssim(x, y)
    check_metrics(x, y)


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("C", [1, 3])
def test_lambda_and_channels(lam, C):
    x, y = pair((C, 45, 70), seed=int(10 * lam) + C, kind="patches")
    check_loss(x, y, lam)


@pytest.mark.parametrize("kind", ["const", "equal"])
def test_constant_and_equal_images(kind):
    x, y = pair((3, 40, 37), seed=3, kind=kind)
    check_loss(x, y, 0.2)
    check_ssim(x, y)
    check_metrics(x, y)


@pytest.mark.parametrize("C", [1, 3])
def test_batches_of_four_per_image(C):
    x, y = pair((4, C, 50, 70), seed=40 + C, kind="patches")
    check_ssim(x, y, size_average=False)
    check_ssim(x, y, size_average=True)
    check_loss(x, y, 0.2)
    check_metrics(x, y)


@pytest.mark.parametrize("H,W", [(528, 800), (1056, 1600)])
def test_full_frames(H, W):
    x, y = pair((3, H, W), seed=H, kind="patches")
    check_loss(x, y, 0.2)
    check_metrics(x, y)


def test_one_image_gradient_only():
    x, y = pair((3, 40, 50), seed=9)
    xg = x.to(DEV).requires_grad_(True)
    photometric.ssim(xg, y.to(DEV)).backward()
    _, gx64, _ = pr.autograd64(pr.ssim64, x, y)
    _, gx32, _ = autograd32(ssim32, x, y)
    within(xg.grad, gx32, gx64, "d ssim / d img1 alone")
    yg = y.to(DEV).requires_grad_(True)
    loss, _ = photometric.photometric_loss(x.to(DEV), yg)
    loss.backward()
    _, _, gy64 = pr.autograd64(lambda a, b: pr.loss64(a, b, 0.2), x, y)
    _, _, gy32 = autograd32(lambda a, b: loss32(a, b, 0.2), x, y)
    within(yg.grad, gy32, gy64, "d loss / d gt alone")


def test_non_contiguous_input():
    x, y = pair((60, 50, 3), seed=11)
    xt, yt = x.permute(2, 0, 1), y.permute(2, 0, 1)
    got = photometric.ssim(xt.to(DEV), yt.to(DEV))
    within(got, ssim32(xt.contiguous(), yt.contiguous()), pr.ssim64(xt, yt), "ssim of a permuted view")


def test_bitwise_reproducible():
    x, y = pair((2, 3, 200, 301), seed=5, kind="patches")
    outs = []
    for _ in range(2):
        xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
        loss, terms = photometric.photometric_loss(xg, yg)
        loss.backward()
        m = photometric.image_metrics(x.to(DEV), y.to(DEV))
        outs.append([loss.detach(), terms.l1, terms.ssim, xg.grad, yg.grad, m.ssim, m.psnr, m.l1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_no_host_synchronisation():
    x, y = pair((3, 64, 96), seed=6)
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    photometric.photometric_loss(xg, yg)  # loads the library and warms up outside the checked region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, terms = photometric.photometric_loss(xg, yg)
        loss.backward()
        s = photometric.ssim(xg, yg)
        s.backward()
        photometric.image_metrics(xg.detach(), yg.detach())
        photometric.psnr(xg.detach(), yg.detach())
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_render_photometric_loss_backward_matches_reference_formula():
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera, make_scene
    sc = make_scene(4000, S=16, sh_degree=3, seed=2, log_scale_mean=-2.6)
    cam = TorchCamera(make_camera(160, 112, yaw=0.2), DEV)
    bg = torch.zeros(3, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    gt = torch.rand(3, 112, 160, device=DEV, generator=g)
    grads = []
    for fused in (True, False):
        pc = GaussianSet.from_scene(sc, DEV)
        image = render(cam, pc, PipelineParams(), bg)["render"]
        if fused:
            loss, _ = photometric.photometric_loss(image, gt, 0.2)
        else:
            loss = loss32_device(image, gt, 0.2)
        loss.backward()
        grads.append({n: p.grad.detach().clone() for n, p in pc.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and grads[0]
    assert float(grads[1]["_xyz"].abs().max()) > 0
    for n in grads[1]:
        a, b = grads[0][n], grads[1][n]
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-3 * scale, n


def loss32_device(image, gt, lam):
    """train.py:137-140 through the reference's F.conv2d ssim, on the device"""
    w = pr.window_2d().to(image.device).expand(3, 1, 11, 11).contiguous()
    conv = lambda t: torch.nn.functional.conv2d(t, w, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(image), conv(gt)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11, s22, s12 = conv(image * image) - mu1_sq, conv(gt * gt) - mu2_sq, conv(image * gt) - mu1_mu2
    m = ((2 * mu1_mu2 + pr.C1) * (2 * s12 + pr.C2)) / ((mu1_sq + mu2_sq + pr.C1) * (s11 + s22 + pr.C2))
    return (1.0 - lam) * torch.abs(image - gt).mean() + lam * (1.0 - m.mean())
