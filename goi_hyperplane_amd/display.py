"""The viewer's frame composed on the device (csrc/display.hip): the stage between a render with its decoded similarity
and the picture the user sees, which the reference runs on the host in numpy on every displayed frame.

    compose               test_step's mode selection, depth normalisation and clamp      gui/main.py:564-587
                          set_clip_mask / render_video: clip_color, cmap and the blend    gui/main.py:387-398, 1788-1800
                                                                                          utils/image_utils.py:129-178
    from_reference_flags  the GUI's three booleans (sim_coloring, res_finetuned, sim_binary) -> a style
    turbo_colormap        matplotlib's Turbo table as the reference loads it (image_utils.py:129)

Arithmetic per view, every operation one float32 rounding in the order written (tests/display_reference.py restates it
in numpy, and tests/golden/ref_display_pins.npz pins it to the reference's own functions bit for bit):

    base = image [C, H, W], C in {1, 3}; C == 1 is repeated to three channels (depth / alpha modes)
    normalize:  base = (base - min) / ((max - min) + f32(1e-20))           min / max over the view
    base = clamp(base, 0, 1)
    NONE      out = base
    BINARY    out = sim > 0 ? 1 : 0
    WHITEN    col = 1;  a = bg ? 1 : 0;  opa = a * f32(ratio);  om = 1 - opa
    HEAT      rel = clamp(((sim - f32(t)) - f32(0.05)) / (max(sim) - f32(t)), 0, 1)
              col = bg ? 1 : clamp(table[(long)(rel * f32(K - 1))], 0, 1);  opa = f32(ratio);  om = f32(1.0 - ratio)
    HEAT_FT   rel = clamp(sim + f32(0.2), 0.1, 0.9);  col as HEAT;  a = bg ? 1 : 0;  opa = a * f32(ratio);  om = 1 - opa
    overlay   out = clamp(col * opa + base * om, 0, 1)
    uint8     out = (uint8)(out * f32(255)), truncated

In HEAT the reference's alpha is the Python int 1, so its `1 - opa` is a Python float: the subtraction is made in double
and rounded to float32 once.  In WHITEN and HEAT_FT alpha is a float32 array and everything stays in float32.

A NaN similarity makes the reference raise (the table index is undefined); here its colour is table entry 0 and it is
skipped by the maximum.  The sign of a zero in the output is not specified.  Everything is asynchronous on the current
stream: at most two kernel launches whatever the number of views, and nothing is read back to the host.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check, ptr, stream

# GOI_FRAME_* of include/goi_raster.h
NONE, BINARY, WHITEN, HEAT, HEAT_FT = 0, 1, 2, 3, 4
STYLES = {"none": NONE, "binary": BINARY, "whiten": WHITEN, "heat": HEAT, "heat_ft": HEAT_FT}
MAX_COLORS = 1024  # GOI_FRAME_MAX_COLORS: the table is staged in LDS
_F32, _U8 = 0, 1  # GOI_FRAME_F32, GOI_FRAME_U8
_TURBO = {}  # device -> the Turbo table, built once
_NO_CPU = "goi_hyperplane_amd.display: tensors must live on a ROCm GPU; there is no CPU fallback"


def from_reference_flags(coloring: bool, res_finetuned: bool, sim_binary: bool) -> int:
    """The style the reference's viewer shows for its three switches (gui/main.py:391-398 with clip_color): sim_binary
    wins; without sim_coloring the background is whitened whatever res_finetuned says; with it the heat map takes the
    fine-tuned or the thresholded relevancy."""
    if sim_binary:
        return BINARY
    if not coloring:
        return WHITEN
    return HEAT_FT if res_finetuned else HEAT


def turbo_colormap(device) -> torch.Tensor:
    """matplotlib's Turbo table as float32 [256, 3] on `device`: the reference's
    torch.tensor(matplotlib.colormaps.get_cmap('turbo').colors).  The package does not ship the table: without matplotlib
    this raises, and any float32 [K, 3] table can be passed to compose instead.  The tensor is built once per device and
    shared: do not write to it."""
    try:
        import matplotlib
    except ImportError as ex:
        raise RuntimeError("display.turbo_colormap needs matplotlib (the table is not shipped with this package); pass "
                           "your own float32 [K, 3] colour table as compose(..., colormap=table)") from ex
    key = str(torch.device(device))
    if key not in _TURBO:  # one host -> device copy per device, not one per frame
        _TURBO[key] = torch.tensor(matplotlib.colormaps.get_cmap("turbo").colors, dtype=torch.float32, device=device)
    return _TURBO[key]


def _style(style) -> int:
    if isinstance(style, str):
        if style not in STYLES:
            raise ValueError(f"compose: unknown style {style!r}; expected one of {sorted(STYLES)}")
        return STYLES[style]
    if isinstance(style, bool) or not isinstance(style, int) or not NONE <= style <= HEAT_FT:
        raise ValueError(f"compose: unknown style {style!r}; expected display.NONE .. display.HEAT_FT or a name")
    return style


def compose(base: torch.Tensor, sim: torch.Tensor | None = None, bg_mask: torch.Tensor | None = None, *, style,
            normalize: bool = False, overlay_ratio: float = 1.0, heat_thresh: float = 0.7,
            colormap: torch.Tensor | None = None, dtype: torch.dtype = torch.float32,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """The displayed frame(s) of `base` [C, H, W] or [V, C, H, W] (float32, C in {1, 3}) -> [H, W, 3] or [V, H, W, 3] of
    `dtype` (torch.float32, what the viewer's texture takes, or torch.uint8, what render_video saves); see the module
    docstring for the arithmetic.

    sim       float32 similarity per pixel, [H*W], [H, W] or [V, ...] of V*H*W elements (BINARY, HEAT, HEAT_FT)
    bg_mask   bool / uint8 of the same pixels, nonzero = background (WHITEN, HEAT, HEAT_FT)
    style     display.NONE / BINARY / WHITEN / HEAT / HEAT_FT or "none" / "binary" / "whiten" / "heat" / "heat_ft"
    normalize the min-max normalisation of test_step's depth mode, over each view
    overlay_ratio, heat_thresh   the viewer's color_overlay_ratio and clip_color's thresh (0.7 at both call sites)
    colormap  float32 [K, 3], 2 <= K <= MAX_COLORS (HEAT, HEAT_FT); None: turbo_colormap(base.device)
    out       a contiguous tensor of the result's shape and dtype to write into

    In a batch every view takes its own minimum and maximum.  CUDA tensors only; arguments are checked on the host before
    anything is launched."""
    code = _style(style)
    if not isinstance(base, torch.Tensor):
        raise TypeError(f"compose: base must be a tensor, got {type(base).__name__}")
    if base.dtype != torch.float32:
        raise TypeError(f"compose: base must be float32, got {base.dtype}")
    if base.dim() not in (3, 4):
        raise ValueError(f"compose: base must be [C, H, W] or [V, C, H, W], got shape {tuple(base.shape)}")
    batched = base.dim() == 4
    V = int(base.shape[0]) if batched else 1
    Cc, H, W = (int(d) for d in base.shape[-3:])
    if Cc not in (1, 3):
        raise ValueError(f"compose: base must have 1 or 3 channels, got {Cc}")
    if H < 1 or W < 1 or V < 1 or H * W >= 2 ** 31 or V > 65535:
        raise ValueError(f"compose: need 1 <= V <= 65535 views of H, W >= 1 with H * W < 2^31, got {V} of {H}x{W}")
    if dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"compose: dtype must be torch.float32 or torch.uint8, got {dtype}")
    heat = code in (HEAT, HEAT_FT)
    need_sim, need_bg = heat or code == BINARY, heat or code == WHITEN
    if need_sim:
        if sim is None:
            raise ValueError("compose: this style needs sim")
        if sim.dtype != torch.float32:
            raise TypeError(f"compose: sim must be float32, got {sim.dtype}")
        if sim.numel() != V * H * W:
            raise ValueError(f"compose: sim has {sim.numel()} elements, {V} view(s) of {H}x{W} need {V * H * W}")
    if need_bg:
        if bg_mask is None:
            raise ValueError("compose: this style needs bg_mask")
        if bg_mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"compose: bg_mask must be bool or uint8, got {bg_mask.dtype}")
        if bg_mask.numel() != V * H * W:
            raise ValueError(f"compose: bg_mask has {bg_mask.numel()} elements, {V} view(s) of {H}x{W} need {V * H * W}")
    ratio, thresh = float(overlay_ratio), float(heat_thresh)
    if ratio != ratio or thresh != thresh:
        raise ValueError("compose: overlay_ratio and heat_thresh must not be NaN")
    if heat and colormap is not None:
        if not isinstance(colormap, torch.Tensor) or colormap.dtype != torch.float32:
            raise TypeError("compose: colormap must be a float32 tensor [K, 3]")
        if colormap.dim() != 2 or colormap.shape[1] != 3 or not 2 <= colormap.shape[0] <= MAX_COLORS:
            raise ValueError(f"compose: colormap must be [K, 3] with 2 <= K <= {MAX_COLORS}, got shape {tuple(colormap.shape)}")
    shape = (V, H, W, 3) if batched else (H, W, 3)
    if out is not None and (tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous()):
        raise ValueError(f"compose: out must be a contiguous {dtype} tensor of shape {shape}, got {out.dtype} {tuple(out.shape)}")
    used = [base] + ([sim] if need_sim else []) + ([bg_mask] if need_bg else []) + ([out] if out is not None else []) \
        + ([colormap] if heat and colormap is not None else [])
    if not all(t.is_cuda for t in used):
        raise RuntimeError(_NO_CPU)
    dev = base.device
    if any(t.device != dev for t in used):
        raise ValueError("compose: all tensors must live on one device")

    lib = _lib.load()
    table = None
    if heat:
        table = (turbo_colormap(dev) if colormap is None else colormap).contiguous()
    src = base.contiguous()
    s = sim.contiguous() if need_sim else None
    m = None
    if need_bg:
        m = bg_mask.contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else m
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    need_ws = (normalize and code != BINARY) or code == HEAT
    ws = torch.empty((V, 3), dtype=torch.int32, device=dev) if need_ws else None
    with torch.cuda.device(dev):
        check(lib.goi_semantic_frame_compose(ptr(src), Cc, ptr(s), ptr(m), V, H, W, code, 1 if normalize else 0, ratio, thresh,
                                             ptr(table), 0 if table is None else int(table.shape[0]), ptr(out),
                                             _U8 if dtype == torch.uint8 else _F32, ptr(ws), stream(dev)))
    return out
