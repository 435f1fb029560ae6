"""Writes ref_photometric_pins.npz: the reference's own photometric functions in fp32 on the CPU -- loss_utils.ssim and
loss_utils.l1_loss imported from the reference checkout, image_utils.psnr executed from its AST (the module imports cv2
and torchvision) -- with autograd gradients with respect to both images of

    ssim(x, y)                                     (ssim_gx, ssim_gy)
    (1 - 0.2) * l1_loss(x, y) + 0.2 * (1 - ssim)   (loss_gx, loss_gy; train.py:137-140 with lambda_dssim = 0.2)

Cases: hw [3, 37, 53] with an x == y block, batch [2, 3, 64, 80] (also ssim with size_average=False), tiny [3, 4, 6]
(smaller than the window), const (x a constant image) and equal (x == y everywhere).  Images are multiples of 1/255 and
stored as uint8 codes; the batch keeps only its loss gradients, to keep the file small.

    python tests/golden/make_photometric_golden.py  (needs the reference checkout; set GOI_REFERENCE to its path)"""
import ast
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GOI_REFERENCE", "/root/reference")
LAMBDA = 0.2


def reference_loss_utils():
    spec = importlib.util.spec_from_file_location("ref_loss_utils", os.path.join(REF, "utils", "loss_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_psnr():
    src = open(os.path.join(REF, "utils", "image_utils.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "psnr")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "image_utils.py:psnr", "exec"), ns)
    return ns["psnr"]


def codes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.int64).to(torch.uint8)


def cases():
    """name -> (x codes, y codes) as uint8 arrays; images are codes / 255"""
    out = {}
    x, y = codes((3, 37, 53), 1), codes((3, 37, 53), 2)
    y[:, 5:20, 10:30] = x[:, 5:20, 10:30]
    out["hw"] = (x, y)
    out["batch"] = (codes((2, 3, 64, 80), 3), codes((2, 3, 64, 80), 4))
    out["tiny"] = (codes((3, 4, 6), 5), codes((3, 4, 6), 6))
    out["const"] = (torch.full((3, 24, 20), 128, dtype=torch.uint8), codes((3, 24, 20), 7))
    e = codes((3, 16, 20), 8)
    out["equal"] = (e, e.clone())
    return {k: (a.numpy(), b.numpy()) for k, (a, b) in out.items()}


def image(c):
    return torch.from_numpy(c).float() / 255


def main():
    lu, psnr = reference_loss_utils(), reference_psnr()
    out = {"lambda_dssim": LAMBDA}
    for name, (xc, yc) in cases().items():
        out[f"{name}_x"], out[f"{name}_y"] = xc, yc
        x = image(xc).requires_grad_(True)
        y = image(yc).requires_grad_(True)
        s = lu.ssim(x, y)
        l1 = lu.l1_loss(x, y)
        loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - s)
        out[f"{name}_ssim"], out[f"{name}_l1"], out[f"{name}_loss"] = s.item(), l1.item(), loss.item()
        out[f"{name}_psnr"] = psnr(x.detach(), y.detach()).numpy()
        if name != "batch":
            gx, gy = torch.autograd.grad(s, (x, y), retain_graph=True)
            out[f"{name}_ssim_gx"], out[f"{name}_ssim_gy"] = gx.numpy(), gy.numpy()
        else:
            out[f"{name}_ssim_per_image"] = lu.ssim(x, y, size_average=False).detach().numpy()
        gx, gy = torch.autograd.grad(loss, (x, y))
        out[f"{name}_loss_gx"], out[f"{name}_loss_gy"] = gx.numpy(), gy.numpy()
    path = os.path.join(HERE, "ref_photometric_pins.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
