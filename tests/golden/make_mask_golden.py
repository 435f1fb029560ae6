"""Writes tests/golden/ref_mask_metric_pins.npz: the reference's own segmentation metrics (utils/image_utils.py:59-102:
calculate_iou, calculate_mean_pixel_accuracy, calculate_mean_precision) on crafted mask pairs, evaluated by importing
that module from a checkout of the reference (the tests only read the file).

cv2 and torchvision are imported by the module but not used by the three functions; they are stubbed in sys.modules so
that neither has to be installed, and the colour map the module places on "cuda" at import is placed on the host.
The masks are stored bit-packed (np.packbits of the flattened [H, W] masks), with the metrics as the reference returns
them: iou a Python float (float64 here, NaN for an empty union), mPA and mP float32 0-d tensors.
`big_counts` has more than 2^24 pixels in a class, so the float32 rounding of the counts shows.

    python tests/golden/make_mask_golden.py /path/to/reference/checkout
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_mask_metric_pins.npz")


def reference_metrics(ref_root):
    for name in ("cv2", "torchvision", "torchvision.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    # the module builds a colour map tensor on "cuda" at import; the generator needs no GPU, so that one lands on the host
    real_tensor = torch.tensor
    torch.tensor = lambda *a, **k: real_tensor(*a, **{**k, "device": "cpu"})
    sys.path.insert(0, ref_root)
    try:
        mod = importlib.import_module("utils.image_utils")
    finally:
        sys.path.remove(ref_root)
        torch.tensor = real_tensor
    return mod.calculate_iou, mod.calculate_mean_pixel_accuracy, mod.calculate_mean_precision


def cases():
    rng = np.random.default_rng(20261015)
    H, W = 48, 80
    z = np.zeros((H, W), bool)
    rand = lambda p, h=H, w=W: rng.random((h, w)) < p  # noqa: E731
    out = {
        "empty_gt": (rand(0.3), z.copy()),
        "empty_pred": (z.copy(), rand(0.3)),
        "both_empty": (z.copy(), z.copy()),
        "both_full": (~z, ~z),
    }
    left, right = z.copy(), z.copy()
    left[:, :30], right[:, 50:] = True, True
    out["disjoint"] = (left, right)
    one_p, one_g = z.copy(), z.copy()
    one_p[7, 65], one_g[7, 65] = True, True
    out["single_pixel"] = (one_p, one_g)
    miss_p, miss_g = z.copy(), z.copy()
    miss_p[0, 0], miss_g[H - 1, W - 1] = True, True
    out["single_pixel_missed"] = (miss_p, miss_g)
    out["random_512_sparse"] = (rand(0.02, 512, 512), rand(0.05, 512, 512))
    out["random_512_dense"] = (rand(0.5, 512, 512), rand(0.45, 512, 512))
    out["random_528x800"] = (rand(0.3, 528, 800), rand(0.3, 528, 800))
    # 4200 x 4200 = 17 640 000 pixels: TN and the class-0 totals lie above 2^24, where float32 keeps only even integers
    Hb = Wb = 4200
    flat_p, flat_g = np.zeros(Hb * Wb, bool), np.zeros(Hb * Wb, bool)
    flat_p[5001: 5001 + 33334] = True
    flat_g[1000: 1000 + 12345] = True
    flat_g[20000: 20000 + 7778] = True
    out["big_counts"] = (flat_p.reshape(Hb, Wb), flat_g.reshape(Hb, Wb))
    return out


def main(ref_root):
    calc_iou, calc_mpa, calc_mp = reference_metrics(ref_root)
    data = {}
    names = []
    for name, (pred, gt) in cases().items():
        names.append(name)
        p, g = torch.from_numpy(pred), torch.from_numpy(gt)
        iou = calc_iou(g, p)  # eval_epoch's argument order: (ground truth, prediction)
        mpa = calc_mpa(g, p)
        mp = calc_mp(g, p)
        assert isinstance(iou, float) and mpa.dtype == torch.float32 and mp.dtype == torch.float32
        data[f"{name}_shape"] = np.array(pred.shape, np.int64)
        data[f"{name}_pred"] = np.packbits(pred.reshape(-1))
        data[f"{name}_gt"] = np.packbits(gt.reshape(-1))
        data[f"{name}_iou"] = np.float64(iou)
        data[f"{name}_mpa"] = np.float32(mpa.item())
        data[f"{name}_mp"] = np.float32(mp.item())
        print(f"{name:22s} iou {iou!r:24} mpa {mpa.item()!r:22} mp {mp.item()!r}")
    data["cases"] = np.array(names)
    np.savez_compressed(OUT, **data)
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
