"""Writes tests/golden/ref_display_pins.npz: the frames the reference's viewer shows, computed by the reference's own
functions on seeded inputs (the tests only read the file).

The module utils/image_utils.py of a checkout of the reference is imported and ITS clip_color and cmap are run, with the
callers' lines around them restated here as they stand in gui/main.py:
    test_step      :564-587   mode selection, the depth normalisation in torch, permute / clamp / numpy
    set_clip_mask  :391-398   opa = alpha * ratio; (colored * opa + image * (1 - opa)).clip(0, 1); the binary mask
    render_video   :1800      (final * 255).astype('uint8')
cv2 and torchvision are imported by the module but not used by these functions; they are stubbed in sys.modules, and
the colour map tensor the module places on "cuda" at import is placed on the host (the generator needs no GPU).

Stored: the inputs of every case, the Turbo table the module built, and for every case x style x ratio the float32 and
the uint8 frame.  Styles: none, binary, whiten (coloring=False), heat (coloring=True), heat_ft (coloring=True,
res_finetuned=True).  Cases: a mixed view with base values below 0 and above 1; an all-background view (max(sim) = 0, so
the heat denominator is negative); a view without background; a view whose maximum equals the heat threshold (the
division gives -inf and clamps to 0); depth mode on a random and on a constant map; alpha mode; an odd-sized view.

    python tests/golden/make_display_golden.py /path/to/reference/checkout
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_display_pins.npz")
RATIOS = (0.0, 0.3, 1.0, 0.6)  # at 0.6 float32(1.0 - r) and float32(1) - float32(r) differ: the heat style takes the former
THRESH = 0.7  # clip_color's thresh at both call sites
# style -> (sim_coloring, res_finetuned, sim_binary) of the GUI; "none" is test_step without a prompt
STYLES = {"none": None, "binary": (False, False, True), "whiten": (False, False, False), "heat": (True, False, False),
          "heat_ft": (True, True, False)}


def reference_module(ref_root):
    for name in ("cv2", "torchvision", "torchvision.transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    real_tensor = torch.tensor
    torch.tensor = lambda *a, **k: real_tensor(*a, **{**k, "device": "cpu"})
    sys.path.insert(0, ref_root)
    try:
        mod = importlib.import_module("utils.image_utils")
    finally:
        sys.path.remove(ref_root)
        torch.tensor = real_tensor
    return mod


def cases():
    """name -> (render [C, H, W] float32, mode, sim [H*W] float32 with its background zeroed, bg [H*W] bool)"""
    rng = np.random.default_rng(20261017)
    H, W = 12, 20

    def decoded(h, w, lo=0.0, hi=1.0, cut=0.5):
        s = rng.uniform(lo, hi, h * w).astype(np.float32)
        bg = s < np.float32(cut)  # compute_similarity: _bg_mask = sim < thresh; sim[_bg_mask] = 0
        s[bg] = 0
        return s, bg

    image = lambda h, w: rng.uniform(-0.3, 1.3, (3, h, w)).astype(np.float32)  # noqa: E731
    out = {}
    out["mixed"] = (image(H, W), "image") + decoded(H, W)
    out["all_background"] = (image(H, W), "image", np.zeros(H * W, np.float32), np.ones(H * W, bool))
    out["no_background"] = (image(H, W), "image") + decoded(H, W, 0.5, 1.0)
    s, bg = decoded(H, W, 0.0, 0.7)
    s[~bg] = np.minimum(s[~bg], np.float32(THRESH))
    s[np.flatnonzero(~bg)[:5]] = np.float32(THRESH)
    assert s.max() == np.float32(THRESH)
    out["max_equals_thresh"] = (image(H, W), "image", s, bg)
    out["depth"] = (rng.uniform(0.5, 9.0, (1, H, W)).astype(np.float32), "depth") + decoded(H, W)
    out["depth_constant"] = (np.full((1, H, W), 2.5, np.float32), "depth") + decoded(H, W)
    out["alpha"] = (rng.uniform(0.0, 1.0, (1, H, W)).astype(np.float32), "alpha") + decoded(H, W)
    out["odd_7x9"] = (image(7, 9), "image") + decoded(7, 9)
    return out


def step_image(render, mode):
    """gui/main.py:564-587 (F.interpolate to the render's own size is the identity and is left out)"""
    buffer_image = torch.from_numpy(render)
    if mode in ["depth", "alpha"]:
        buffer_image = buffer_image.repeat(3, 1, 1)
        if mode == "depth":
            buffer_image = (buffer_image - buffer_image.min()) / (buffer_image.max() - buffer_image.min() + 1e-20)
    return buffer_image.permute(1, 2, 0).contiguous().clamp(0, 1).contiguous().detach().cpu().numpy()


def set_clip_mask(mod, buffer_image, cos_sim, bg_mask, H, W, flags, color_overlay_ratio):
    """gui/main.py:391-398"""
    sim_coloring, res_finetuned, sim_binary = flags
    if not sim_binary:
        colored_img, alpha = mod.clip_color(cos_sim, bg_mask, height=H, width=W, thresh=0.7, res_finetuned=res_finetuned,
                                            coloring=sim_coloring, device="cpu")
        opa = alpha * color_overlay_ratio
        return (colored_img * opa + buffer_image * (1 - opa)).clip(0, 1)
    mask = cos_sim > 0
    binary_mask = mask.reshape(H, W).float().unsqueeze(-1).repeat(1, 1, 3)
    return binary_mask.contiguous().clamp(0, 1).contiguous().detach().cpu().numpy()


def main(ref_root):
    mod = reference_module(ref_root)
    data = {"table": mod.turbo_colormap.numpy().astype(np.float32), "ratios": np.array(RATIOS, np.float64),
            "thresh": np.float64(THRESH), "styles": np.array(list(STYLES))}
    assert data["table"].shape == (256, 3)
    names = []
    for name, (render, mode, sim, bg) in cases().items():
        names.append(name)
        _, H, W = render.shape
        data[f"{name}__base"], data[f"{name}__sim"], data[f"{name}__bg"] = render, sim, bg
        data[f"{name}__mode"] = np.array(mode)
        for style, flags in STYLES.items():
            for k, ratio in enumerate(RATIOS):
                buffer_image = step_image(render, mode)
                if flags is not None:
                    final = set_clip_mask(mod, buffer_image, torch.from_numpy(sim.copy()), torch.from_numpy(bg.copy()), H, W,
                                          flags, ratio)
                else:
                    final = buffer_image
                final = np.broadcast_to(final, (H, W, 3))
                assert final.dtype == np.float32, (name, style, final.dtype)
                data[f"{name}__{style}__{k}__f32"] = np.ascontiguousarray(final)
                data[f"{name}__{style}__{k}__u8"] = (final * 255).astype("uint8")
    data["cases"] = np.array(names)
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(names), "cases")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
