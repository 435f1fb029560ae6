"""The viewer's frame stage without a GPU: the numpy restatement (tests/display_reference.py) reproduces the frames the
reference's own clip_color / cmap and callers produced (tests/golden/ref_display_pins.npz, written by
tests/golden/make_display_golden.py) bit for bit, float32 and uint8; the pins cover every style, both dtypes and the
edge cases; display.compose refuses bad arguments on the host and CPU tensors loudly."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests import display_reference as ref

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_display_pins.npz")
STYLE_CODES = {"none": ref.NONE, "binary": ref.BINARY, "whiten": ref.WHITEN, "heat": ref.HEAT, "heat_ft": ref.HEAT_FT}


@pytest.fixture(scope="module")
def pins():
    with np.load(PINS) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def pinned_frames(pins):
    """(case, style name, ratio, uint8?, expected frame, restatement arguments) of every pinned frame"""
    for case in pins["cases"]:
        base, sim, bg = pins[f"{case}__base"], pins[f"{case}__sim"], pins[f"{case}__bg"]
        normalize = str(pins[f"{case}__mode"]) == "depth"
        for style in pins["styles"]:
            for k, ratio in enumerate(pins["ratios"]):
                for u8 in (False, True):
                    want = pins[f"{case}__{style}__{k}__{'u8' if u8 else 'f32'}"]
                    kw = dict(style=STYLE_CODES[str(style)], normalize=normalize, ratio=float(ratio),
                              thresh=float(pins["thresh"]), table=pins["table"], uint8=u8)
                    yield str(case), str(style), float(ratio), u8, want, (base, sim, bg, kw)


def test_restatement_reproduces_every_pin_bit_for_bit(pins):
    n = 0
    for case, style, ratio, u8, want, (base, sim, bg, kw) in pinned_frames(pins):
        got = ref.compose(base, sim, bg, **kw)
        assert got.dtype == want.dtype and got.shape == want.shape, (case, style, ratio, u8)
        assert np.array_equal(bits(got), bits(want)), (case, style, ratio, u8, int((bits(got) != bits(want)).sum()))
        n += 1
    assert n == len(pins["cases"]) * 5 * 4 * 2


def test_pins_cover_every_style_dtype_and_edge_case(pins):
    assert set(map(str, pins["styles"])) == set(STYLE_CODES)
    assert list(pins["ratios"]) == [0.0, 0.3, 1.0, 0.6]
    assert pins["table"].shape == (256, 3) and pins["table"].dtype == np.float32
    cases = set(map(str, pins["cases"]))
    assert {"mixed", "all_background", "no_background", "max_equals_thresh", "depth", "depth_constant", "alpha",
            "odd_7x9"} <= cases
    for case in cases:
        for style in STYLE_CODES:
            for k in range(4):
                assert pins[f"{case}__{style}__{k}__f32"].dtype == np.float32
                assert pins[f"{case}__{style}__{k}__u8"].dtype == np.uint8
        C, H, W = pins[f"{case}__base"].shape
        assert H <= 64 and W <= 96
    thresh = np.float32(pins["thresh"])
    assert pins["all_background__bg"].all() and pins["all_background__sim"].max() == 0  # the heat denominator is negative
    assert not pins["no_background__bg"].any()
    assert pins["max_equals_thresh__sim"].max() == thresh  # -inf, clamped to 0: every foreground pixel takes table[0]
    fg = ~pins["max_equals_thresh__bg"].reshape(12, 20)
    assert fg.any() and np.array_equal(pins["max_equals_thresh__heat__2__f32"][fg],
                                       np.broadcast_to(pins["table"][0], (int(fg.sum()), 3)))
    assert pins["mixed__base"].min() < 0 and pins["mixed__base"].max() > 1
    d = pins["depth_constant__base"]
    assert d.shape[0] == 1 and d.min() == d.max() and str(pins["depth_constant__mode"]) == "depth"
    assert not pins["depth_constant__none__0__f32"].any()  # 0 / (0 + 1e-20)
    assert pins["depth__none__0__f32"].max() == 1.0 and str(pins["alpha__mode"]) == "alpha"
    assert pins["odd_7x9__base"].shape == (3, 7, 9)
    # the ratios matter where they should and the three overlay styles differ from one another
    assert not np.array_equal(pins["mixed__heat__1__f32"], pins["mixed__heat__2__f32"])
    assert not np.array_equal(pins["mixed__heat__1__f32"], pins["mixed__heat_ft__1__f32"])
    # the reference's fine-tuned heat map is opaque only where the colour is the background's white: it shows what the
    # whitened style shows (clip_color returns both the heat image and the background alpha when res_finetuned is set)
    assert np.array_equal(pins["mixed__whiten__1__f32"], pins["mixed__heat_ft__1__f32"])
    assert not np.array_equal(pins["mixed__whiten__1__f32"], pins["mixed__none__1__f32"])
    assert np.array_equal(pins["mixed__heat__0__f32"], pins["mixed__none__0__f32"])  # ratio 0 shows the image


def test_double_one_minus_ratio_is_what_the_reference_does(pins):
    """For ratio 0.6 the host's 1 - ratio (double, then float32) and float32(1) - float32(ratio) differ by an ulp, and the
    pinned heat frame follows the former: blending with the latter gives other bits."""
    r = float(pins["ratios"][3])
    assert r == 0.6 and np.float32(1.0 - r) != np.float32(1) - np.float32(r)
    base, sim, bg = pins["mixed__base"], pins["mixed__sim"], pins["mixed__bg"]
    want = pins["mixed__heat__3__f32"]
    assert np.array_equal(bits(ref.compose(base, sim, bg, style=ref.HEAT, ratio=r, table=pins["table"])), bits(want))
    col = ref.compose(base, sim, bg, style=ref.HEAT, ratio=1.0, table=pins["table"])  # ratio 1: the colour alone
    b = np.clip(base, 0, 1).transpose(1, 2, 0)
    wrong = np.clip(col * np.float32(r) + b * (np.float32(1) - np.float32(r)), np.float32(0), np.float32(1))
    assert not np.array_equal(bits(wrong), bits(want))


def test_from_reference_flags():
    from goi_hyperplane_amd import display
    assert display.from_reference_flags(False, False, True) == display.BINARY
    assert display.from_reference_flags(True, True, True) == display.BINARY
    assert display.from_reference_flags(False, False, False) == display.WHITEN
    assert display.from_reference_flags(False, True, False) == display.WHITEN
    assert display.from_reference_flags(True, False, False) == display.HEAT
    assert display.from_reference_flags(True, True, False) == display.HEAT_FT
    assert (display.NONE, display.BINARY, display.WHITEN, display.HEAT, display.HEAT_FT) == \
        (ref.NONE, ref.BINARY, ref.WHITEN, ref.HEAT, ref.HEAT_FT)


def test_header_defines_match_the_python_constants():
    import re
    from goi_hyperplane_amd import display
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(PINS)), "..", "include", "goi_raster.h")).read()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))  # noqa: E731
    assert [val(f"GOI_FRAME_{n}") for n in ("NONE", "BINARY", "WHITEN", "HEAT", "HEAT_FT")] == \
        [display.NONE, display.BINARY, display.WHITEN, display.HEAT, display.HEAT_FT]
    assert (val("GOI_FRAME_F32"), val("GOI_FRAME_U8")) == (display._F32, display._U8)
    assert val("GOI_FRAME_MAX_COLORS") == display.MAX_COLORS >= 1024


def test_turbo_colormap_is_the_pinned_table(pins):
    from goi_hyperplane_amd import display
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="needs matplotlib"):
            display.turbo_colormap("cpu")
        return
    t = display.turbo_colormap("cpu")
    assert t.dtype == torch.float32 and np.array_equal(bits(t.numpy()), bits(pins["table"]))


def test_host_side_validation():
    from goi_hyperplane_amd import display
    z = torch.zeros
    img, sim, bg, tab = z(3, 4, 6), z(24), z(24, dtype=torch.bool), z(256, 3)
    ok = dict(style=display.HEAT, colormap=tab)
    with pytest.raises(ValueError, match="unknown style"):
        display.compose(img, sim, bg, style="rainbow")
    with pytest.raises(ValueError, match="unknown style"):
        display.compose(img, sim, bg, style=5)
    with pytest.raises(TypeError, match="base must be float32"):
        display.compose(img.double(), sim, bg, **ok)
    with pytest.raises(ValueError, match=r"\[C, H, W\] or \[V, C, H, W\]"):
        display.compose(z(4, 6), sim, bg, **ok)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        display.compose(z(2, 4, 6), sim, bg, **ok)
    with pytest.raises(TypeError, match="dtype must be"):
        display.compose(img, sim, bg, dtype=torch.float16, **ok)
    with pytest.raises(ValueError, match="needs sim"):
        display.compose(img, None, bg, **ok)
    with pytest.raises(ValueError, match="needs sim"):
        display.compose(img, style=display.BINARY)
    with pytest.raises(ValueError, match="needs bg_mask"):
        display.compose(img, sim, None, style=display.WHITEN)
    with pytest.raises(TypeError, match="sim must be float32"):
        display.compose(img, sim.double(), bg, **ok)
    with pytest.raises(ValueError, match="sim has 23 elements"):
        display.compose(img, z(23), bg, **ok)
    with pytest.raises(TypeError, match="bg_mask must be bool or uint8"):
        display.compose(img, sim, z(24), **ok)
    with pytest.raises(ValueError, match="bg_mask has 48 elements"):
        display.compose(img, sim, z(48, dtype=torch.uint8), **ok)
    with pytest.raises(ValueError, match="colormap must be"):
        display.compose(img, sim, bg, style=display.HEAT, colormap=z(display.MAX_COLORS + 1, 3))
    with pytest.raises(ValueError, match="colormap must be"):
        display.compose(img, sim, bg, style=display.HEAT_FT, colormap=z(1, 3))
    with pytest.raises(ValueError, match="colormap must be"):
        display.compose(img, sim, bg, style=display.HEAT, colormap=z(256, 4))
    with pytest.raises(TypeError, match="colormap must be"):
        display.compose(img, sim, bg, style=display.HEAT, colormap=z(256, 3).double())
    with pytest.raises(ValueError, match="out must be"):
        display.compose(img, sim, bg, out=z(4, 6, 3, dtype=torch.uint8), **ok)
    with pytest.raises(ValueError, match="out must be"):
        display.compose(img, sim, bg, out=z(3, 4, 6), **ok)
    with pytest.raises(ValueError, match="NaN"):
        display.compose(img, sim, bg, overlay_ratio=float("nan"), **ok)


def test_cpu_tensors_are_refused():
    from goi_hyperplane_amd import display
    z = torch.zeros
    for style, args in ((display.NONE, (z(3, 4, 6),)), (display.BINARY, (z(1, 4, 6), z(4, 6))),
                        (display.HEAT, (z(2, 3, 4, 6), z(2, 24), z(2, 4, 6, dtype=torch.uint8)))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            display.compose(*args, style=style, colormap=z(7, 3))


def test_c_abi_refuses_bad_arguments():
    """goi_semantic_frame_compose returns < 0 with a message before anything is launched (the pointers are never read)."""
    import ctypes as C
    from goi_hyperplane_amd import build, _lib
    build.build()
    lib = _lib.load()
    fake = C.c_void_p(1 << 20)

    def call(base=fake, channels=3, sim=fake, bg=fake, n_views=1, H=4, W=6, style=3, normalize=0, ratio=1.0, thresh=0.7,
             table=fake, n_colors=256, out=fake, out_dtype=0, ws=fake):
        return lib.goi_semantic_frame_compose(base, channels, sim, bg, n_views, H, W, style, normalize, ratio, thresh, table,
                                              n_colors, out, out_dtype, ws, None)

    for kw, text in ((dict(H=0), "H >= 1"), (dict(style=5), "unknown style"), (dict(style=-1), "unknown style"),
                     (dict(out_dtype=2), "out_dtype"), (dict(channels=2), "channels"), (dict(n_views=-1), "n_views"),
                     (dict(n_views=65536), "n_views"), (dict(out=None), "NULL base or out"),
                     (dict(base=None, style=0), "NULL base or out"), (dict(sim=None), "needs sim"),
                     (dict(sim=None, style=1), "needs sim"), (dict(bg=None, style=2), "needs bg_mask"),
                     (dict(table=None), "table"), (dict(n_colors=1025), "table"), (dict(n_colors=1), "table"),
                     (dict(ws=None), "NULL workspace"), (dict(ws=None, style=0, normalize=1), "NULL workspace"),
                     (dict(ratio=float("nan")), "NaN")):
        assert call(**kw) < 0, kw
        assert text in lib.goi_raster_last_error().decode(), (kw, lib.goi_raster_last_error().decode())
    assert call(n_views=0) == 0
    assert lib.goi_semantic_frame_workspace_bytes(3) == 36 and lib.goi_semantic_frame_workspace_bytes(0) == 0
