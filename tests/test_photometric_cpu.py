"""CPU checks of the photometric contract (csrc/photometric.hip, goi_hyperplane_amd.photometric).

* the float64 restatement (tests/photometric_reference.py) reproduces the reference's own fp32 values and gradients
  (tests/golden/ref_photometric_pins.npz) to fp32 accuracy;
* the hand-derived backward the kernel implements equals autograd of the restatement;
* the host refuses window sizes other than 11, wrong dtypes, mismatched or wrong-rank shapes, and CPU tensors."""
import os

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import photometric
from tests import photometric_reference as pr

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_photometric_pins.npz")
CASES = ("hw", "batch", "tiny", "const", "equal")


def pins():
    return np.load(GOLD)


def images(z, name):
    return torch.from_numpy(z[f"{name}_x"]).float() / 255, torch.from_numpy(z[f"{name}_y"]).float() / 255


def close(got64, pin, rel=2e-5):
    got64, pin = np.asarray(got64, np.float64), np.asarray(pin, np.float64)
    scale = max(float(np.abs(got64).max()), 1e-30)
    assert got64.shape == pin.shape
    np.testing.assert_allclose(pin, got64, rtol=0, atol=rel * scale + 1e-8)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference_pins(name):
    z = pins()
    x, y = images(z, name)
    lam = float(z["lambda_dssim"])
    close(pr.ssim64(x, y), z[f"{name}_ssim"])
    close(pr.l1_64(x, y), z[f"{name}_l1"])
    close(pr.loss64(x, y, lam), z[f"{name}_loss"])
    p64, ppin = pr.psnr64(x, y).numpy(), z[f"{name}_psnr"]
    assert p64.shape == ppin.shape
    assert np.array_equal(np.isinf(p64), np.isinf(ppin))
    fin = np.isfinite(p64)
    np.testing.assert_allclose(ppin[fin], p64[fin], rtol=1e-5)
    _, gx, gy = pr.autograd64(lambda a, b: pr.loss64(a, b, lam), x, y)
    close(gx, z[f"{name}_loss_gx"], 1e-4)
    close(gy, z[f"{name}_loss_gy"], 1e-4)
    if name == "batch":
        close(pr.ssim64(x, y, size_average=False), z["batch_ssim_per_image"])
    else:
        _, gx, gy = pr.autograd64(pr.ssim64, x, y)
        close(gx, z[f"{name}_ssim_gx"], 1e-4)
        close(gy, z[f"{name}_ssim_gy"], 1e-4)


@pytest.mark.parametrize("shape,size_average", [((1, 3, 37, 53), True), ((2, 1, 20, 33), False), ((1, 3, 4, 6), True),
                                                ((1, 1, 1, 1), True), ((3, 2, 12, 40), False)])
def test_hand_derived_backward_equals_autograd(shape, size_average):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    y = (x + 0.2 * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    y[..., : shape[2] // 2, : shape[3] // 2] = x[..., : shape[2] // 2, : shape[3] // 2]
    _, ax, ay = pr.autograd64(lambda a, b: pr.ssim64(a, b, size_average), x, y)
    hx, hy = pr.ssim_grad_np(x.numpy(), y.numpy(), size_average)
    np.testing.assert_allclose(hx, ax.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(hy, ay.numpy(), rtol=1e-9, atol=1e-12)


def test_window_is_the_reference_window():
    w2 = pr.window_2d()
    assert w2.dtype == torch.float32 and w2.shape == (11, 11)
    assert abs(float(w2.double().sum()) - 1.0) < 1e-6
    assert torch.equal(w2, w2.t())


def test_host_refuses_bad_arguments():
    x = torch.rand(3, 8, 8)
    with pytest.raises(ValueError, match="window_size"):
        photometric.ssim(x, x, window_size=7)
    with pytest.raises(TypeError, match="float32"):
        photometric.ssim(x.double(), x.double())
    with pytest.raises(TypeError, match="float32"):
        photometric.photometric_loss(x.half(), x.half())
    with pytest.raises(ValueError, match="shapes differ"):
        photometric.l1_loss(x, x[:, :7])
    with pytest.raises(ValueError, match=r"\[C, H, W\]"):
        photometric.psnr(x[0], x[0])
    with pytest.raises(ValueError, match="size_average"):
        photometric.ssim(x, x, size_average=False)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        photometric.image_metrics(x, x)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        photometric.photometric_loss(x, x)
