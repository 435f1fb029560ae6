"""numpy restatement of the viewer's frame stage (goi_hyperplane_amd/display.py, csrc/display.hip): test infrastructure.

Every operation is one float32 rounding in the order the reference makes them (gui/main.py:564-587, :387-398, :1788-1800,
utils/image_utils.py:129-178); tests/test_display_cpu.py holds this file to the reference's own functions bit for bit
through tests/golden/ref_display_pins.npz."""
from __future__ import annotations

import numpy as np

NONE, BINARY, WHITEN, HEAT, HEAT_FT = 0, 1, 2, 3, 4
STYLE_NAMES = {NONE: "none", BINARY: "binary", WHITEN: "whiten", HEAT: "heat", HEAT_FT: "heat_ft"}
f32 = np.float32


def compose_view(base, sim, bg, style, normalize=False, ratio=1.0, thresh=0.7, table=None, uint8=False):
    """One view: base float32 [C, H, W] (C in {1, 3}), sim float32 [H*W] or [H, W], bg bool of the same pixels, table
    float32 [K, 3] -> [H, W, 3] float32, or uint8 when `uint8`."""
    base = np.asarray(base, f32)
    C, H, W = base.shape
    if style == BINARY:
        out = np.repeat((np.asarray(sim, f32).reshape(H, W) > 0).astype(f32)[..., None], 3, axis=2)
    else:
        b = np.repeat(base, 3, axis=0) if C == 1 else base
        if normalize:
            mn, mx = b.min(), b.max()
            b = (b - mn) / ((mx - mn) + f32(1e-20))
        b = np.clip(b, f32(0), f32(1)).transpose(1, 2, 0)
        if style == NONE:
            out = b
        else:
            bgm = np.asarray(bg).reshape(H, W).astype(bool)
            a = bgm.astype(f32)[..., None]
            if style == WHITEN:
                col = f32(1)
            else:
                s = np.asarray(sim, f32).reshape(H, W)
                with np.errstate(divide="ignore", invalid="ignore"):
                    if style == HEAT:
                        rel = np.clip(((s - f32(thresh)) - f32(0.05)) / (s.max() - f32(thresh)), f32(0), f32(1))
                    else:
                        rel = np.clip(s + f32(0.2), f32(0.1), f32(0.9))
                K = table.shape[0]
                col = np.asarray(table, f32)[(rel * f32(K - 1)).astype(np.int64)].copy()
                col[bgm] = 1
                col = np.clip(col, f32(0), f32(1))
            if style == HEAT:
                opa, om = f32(ratio), f32(1.0 - float(ratio))  # 1 - ratio in double, as the host's Python float
            else:
                opa = a * f32(ratio)
                om = f32(1) - opa
            out = np.clip(col * opa + b * om, f32(0), f32(1))
    out = np.ascontiguousarray(out, f32)
    assert out.dtype == f32 and out.shape == (H, W, 3)
    return (out * f32(255)).astype(np.uint8) if uint8 else out


def compose(base, sim=None, bg=None, **kw):
    """[C, H, W] -> [H, W, 3]; [V, C, H, W] -> [V, H, W, 3], every view with its own minimum and maximum."""
    base = np.asarray(base, f32)
    if base.ndim == 3:
        return compose_view(base, sim, bg, **kw)
    V = base.shape[0]
    sims = [None] * V if sim is None else np.asarray(sim).reshape(V, -1)
    bgs = [None] * V if bg is None else np.asarray(bg).reshape(V, -1)
    return np.stack([compose_view(base[v], sims[v], bgs[v], **kw) for v in range(V)])
