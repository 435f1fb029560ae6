"""display.compose (csrc/display.hip) and semantic.view_frame / video_frames on the GPU.

Every frame is compared bit for bit (float32 through its uint32 view): with the frames the reference's own functions
produced (tests/golden/ref_display_pins.npz) and, at sizes from one pixel to many workgroups, with the numpy restatement
(tests/display_reference.py) that tests/test_display_cpu.py holds to those pins.  The sizes take H*W % 4 through all four
values (vector path, scalar tail, misaligned views of a batch); a batch has one all-background view, one without
background and one mixed, so a frame made with another view's maximum shows."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests import display_reference as ref

pytestmark = pytest.mark.gpu

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_display_pins.npz")
STYLE_CODES = {"none": ref.NONE, "binary": ref.BINARY, "whiten": ref.WHITEN, "heat": ref.HEAT, "heat_ft": ref.HEAT_FT}
SIZES = [(1, 1), (1, 3), (3, 5), (7, 9), (8, 8), (5, 13), (17, 67), (64, 64), (129, 257), (528, 800)]
RATIO = 0.6  # float32(1.0 - 0.6) != float32(1) - float32(0.6): the double subtraction shows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pins():
    with np.load(PINS) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), "first at", np.argwhere(bad)[0].tolist())


def table_of(K, seed=5):
    return np.random.default_rng(seed).uniform(0, 1, (K, 3)).astype(np.float32)


def views(V, C, H, W, seed):
    """V views: base in [-0.3, 1.3]; a decoded similarity (background zeroed) that is mixed for one view, all background
    for a batch's view 0 and without background for its view 1, the views' maxima far apart."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-0.3, 1.3, (V, C, H, W)).astype(np.float32)
    sim = np.empty((V, H * W), np.float32)
    bg = np.empty((V, H * W), bool)
    for v in range(V):
        kind = "mixed" if V == 1 else ("all", "none", "mixed")[v % 3]
        if kind == "all":
            sim[v], bg[v] = 0, True
        elif kind == "none":
            sim[v], bg[v] = rng.uniform(0.75, 0.8, H * W), False
        else:
            s = rng.uniform(0.0, 1.0, H * W).astype(np.float32)
            bg[v] = s < 0.5
            s[bg[v]] = 0
            sim[v] = s
    return base, sim, bg


def run(dev, base, sim, bg, **kw):
    from goi_hyperplane_amd import display
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    if "colormap" in kw:
        kw["colormap"] = t(kw["colormap"])
    return display.compose(t(base), t(sim), t(bg), **kw)


def test_every_pinned_frame_bit_equal(dev, pins):
    table = torch.from_numpy(pins["table"]).to(dev)
    from goi_hyperplane_amd import display
    n = 0
    for case in pins["cases"]:
        base, sim, bg = (torch.from_numpy(pins[f"{case}__{k}"]).to(dev) for k in ("base", "sim", "bg"))
        normalize = str(pins[f"{case}__mode"]) == "depth"
        for style in pins["styles"]:
            for k, ratio in enumerate(pins["ratios"]):
                for dtype, tag in ((torch.float32, "f32"), (torch.uint8, "u8")):
                    got = display.compose(base, sim, bg, style=str(style), normalize=normalize, overlay_ratio=float(ratio),
                                          heat_thresh=float(pins["thresh"]), colormap=table, dtype=dtype)
                    same(got, pins[f"{case}__{style}__{k}__{tag}"], (str(case), str(style), float(ratio), tag))
                    n += 1
    assert n == len(pins["cases"]) * 5 * 4 * 2


@pytest.mark.parametrize("H,W", SIZES)
def test_against_the_restatement(dev, H, W):
    table = table_of(256)
    for V in (1, 3):
        base, sim, bg = views(V, 3, H, W, seed=1000 * H + W + V)
        if V == 1:
            base, sim, bg = base[0], sim[0], bg[0]
        for style in STYLE_CODES.values():
            for u8 in (False, True):
                got = run(dev, base, sim, bg, style=style, overlay_ratio=RATIO, colormap=table,
                          dtype=torch.uint8 if u8 else torch.float32)
                want = ref.compose(base, sim, bg, style=style, ratio=RATIO, table=table, uint8=u8)
                same(got, want, (H, W, V, ref.STYLE_NAMES[style], u8))


def test_each_view_takes_its_own_maximum(dev):
    """The heat map of a batch's mixed view differs from the one made with the largest maximum of the batch."""
    table = table_of(256)
    base, sim, bg = views(3, 3, 17, 67, seed=3)
    sim[1] *= np.float32(1.5)  # the view without background now holds the batch's maximum
    assert sim[1].max() > sim[2].max() > sim[0].max() == 0
    got = run(dev, base, sim, bg, style=ref.HEAT, overlay_ratio=RATIO, colormap=table).cpu().numpy()
    same(got, ref.compose(base, sim, bg, style=ref.HEAT, ratio=RATIO, table=table), "batch")
    shared = sim[2].copy()
    shared[np.flatnonzero(bg[2])[0]] = sim[1].max()  # a background pixel carrying the other view's maximum
    other = ref.compose_view(base[2], shared, bg[2], style=ref.HEAT, ratio=RATIO, table=table)
    assert not np.array_equal(got[2], other)


@pytest.mark.parametrize("normalize", [False, True])
def test_single_channel_base(dev, normalize):
    """Depth / alpha modes: C == 1 repeated to three channels, with and without the per-view min-max normalisation; one
    view is constant (0 / (0 + 1e-20))."""
    table = table_of(256)
    for (H, W) in ((7, 9), (64, 64), (5, 13)):
        for V in (1, 3):
            base, sim, bg = views(V, 1, H, W, seed=77 + H + V)
            base = base * np.float32(4.0) + np.float32(2.0)  # depths: well outside [0, 1]
            if not normalize:
                base = base / np.float32(8.0)
            base[V - 1] = np.float32(2.5)
            if V == 1:
                base, sim, bg = base[0], sim[0], bg[0]
            for style in (ref.NONE, ref.HEAT, ref.WHITEN):
                for u8 in (False, True):
                    got = run(dev, base, sim, bg, style=style, normalize=normalize, overlay_ratio=0.3, colormap=table,
                              dtype=torch.uint8 if u8 else torch.float32)
                    want = ref.compose(base, sim, bg, style=style, normalize=normalize, ratio=0.3, table=table, uint8=u8)
                    same(got, want, (H, W, V, ref.STYLE_NAMES[style], normalize, u8))


def test_three_channel_normalize(dev):
    base, sim, bg = views(3, 3, 17, 67, seed=9)
    got = run(dev, base * np.float32(3), None, None, style=ref.NONE, normalize=True)
    same(got, ref.compose(base * np.float32(3), style=ref.NONE, normalize=True), "normalize C=3")


@pytest.mark.parametrize("K", [2, 7, 256, 1024])
def test_table_sizes(dev, K):
    table = table_of(K, seed=K)
    base, sim, bg = views(3, 3, 17, 67, seed=K)
    sim[2, ~bg[2]] = np.linspace(0.5, 1.0, int((~bg[2]).sum()), dtype=np.float32)  # rel sweeps the whole table
    for style in (ref.HEAT, ref.HEAT_FT):
        got = run(dev, base, sim, bg, style=style, overlay_ratio=1.0, colormap=table)
        same(got, ref.compose(base, sim, bg, style=style, ratio=1.0, table=table), (K, ref.STYLE_NAMES[style]))
    used = (np.clip((sim[2][~bg[2]] - np.float32(0.7) - np.float32(0.05)) / (sim[2].max() - np.float32(0.7)), 0, 1)
            * np.float32(K - 1)).astype(np.int64)
    assert used.min() == 0 and used.max() >= int(0.8 * (K - 1))  # the formula's 0.05 keeps rel below 1 ...
    # ... unless every similarity lies under the heat threshold: a negative denominator, rel clamps to 1, the last entry
    got = run(dev, base, sim, bg, style=ref.HEAT, overlay_ratio=1.0, heat_thresh=1.5, colormap=table).cpu().numpy()
    same(got, ref.compose(base, sim, bg, style=ref.HEAT, ratio=1.0, thresh=1.5, table=table), (K, "last entry"))
    fg = ~bg[2].reshape(17, 67)
    assert np.array_equal(got[2][fg], np.broadcast_to(table[K - 1], (int(fg.sum()), 3)))


def test_table_above_the_limit_raises(dev):
    from goi_hyperplane_amd import display
    base, sim, bg = views(1, 3, 3, 5, seed=1)
    with pytest.raises(ValueError, match="colormap must be"):
        run(dev, base[0], sim[0], bg[0], style=ref.HEAT, colormap=table_of(display.MAX_COLORS + 1))


def test_uint8_at_one_and_just_below(dev):
    one, below = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0.0))
    vals = np.array([one, below, np.float32(254.0 / 255.0), np.nextafter(np.float32(254.0 / 255.0), np.float32(1.0)),
                     np.float32(0.5), np.float32(1.0 / 255.0), np.nextafter(np.float32(1.0 / 255.0), np.float32(0.0)),
                     np.float32(0.0), np.float32(1e-30), np.float32(1.5), np.float32(-2.0), np.float32(0.99)], np.float32)
    base = np.broadcast_to(vals, (3, 1, 12)).copy()  # [C=3, H=1, W=12]
    got = run(dev, base, None, None, style=ref.NONE, dtype=torch.uint8).cpu().numpy()
    same(got, ref.compose(base, style=ref.NONE, uint8=True), "uint8 edges")
    flat = got[0, :, 0]
    assert flat[0] == 255 and flat[1] == 254 and flat[7] == 0 and flat[8] == 0 and flat[9] == 255 and flat[10] == 0
    # the same through an overlay: white at ratio 1 is exactly 255
    sim, bg = np.zeros(12, np.float32), np.ones(12, bool)
    white = run(dev, base, sim, bg, style=ref.WHITEN, overlay_ratio=1.0, dtype=torch.uint8).cpu().numpy()
    assert (white == 255).all()


def test_out_reuse_and_unaligned_buffers(dev):
    from goi_hyperplane_amd import display
    table = torch.from_numpy(table_of(256)).to(dev)
    base, sim, bg = views(3, 3, 8, 8, seed=4)
    tb, ts, tm = (torch.from_numpy(a).to(dev) for a in (base, sim, bg))
    want = ref.compose(base, sim, bg, style=ref.HEAT, ratio=RATIO, table=table.cpu().numpy())
    out = torch.full((3, 8, 8, 3), -1.0, device=dev)
    ret = display.compose(tb, ts, tm, style=display.HEAT, overlay_ratio=RATIO, colormap=table, out=out)
    assert ret is out
    same(out, want, "out=")
    with pytest.raises(ValueError, match="out must be"):
        display.compose(tb, ts, tm, style=display.HEAT, colormap=table, out=out[:, :, :4])
    # every buffer one element off its 16-byte boundary: the scalar path, the same frames (H*W is a multiple of 4)
    shift = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].reshape(t.shape)  # noqa: E731
    sb, ss, sm = shift(tb), shift(ts), shift(tm)
    assert sb.data_ptr() % 16 == 4 and ss.data_ptr() % 16 == 4 and sm.data_ptr() % 4 == 1 and sb.is_contiguous()
    for dtype, u8 in ((torch.float32, False), (torch.uint8, True)):
        got = display.compose(sb, ss, sm, style=display.HEAT, overlay_ratio=RATIO, colormap=table, dtype=dtype)
        same(got, ref.compose(base, sim, bg, style=ref.HEAT, ratio=RATIO, table=table.cpu().numpy(), uint8=u8), "shifted")
        got = display.compose(sb, None, None, style=display.NONE, normalize=True, dtype=dtype)
        same(got, ref.compose(base, style=ref.NONE, normalize=True, uint8=u8), "shifted normalize")


def test_two_runs_are_bit_identical(dev):
    table = table_of(256)
    base, sim, bg = views(3, 1, 129, 257, seed=6)
    a = run(dev, base, sim, bg, style=ref.HEAT, normalize=True, overlay_ratio=RATIO, colormap=table)
    b = run(dev, base, sim, bg, style=ref.HEAT, normalize=True, overlay_ratio=RATIO, colormap=table)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    same(a, ref.compose(base, sim, bg, style=ref.HEAT, normalize=True, ratio=RATIO, table=table), "normalised heat")


def test_compose_never_synchronises(dev):
    from goi_hyperplane_amd import display
    table = torch.from_numpy(table_of(256)).to(dev)
    base, sim, bg = views(3, 1, 17, 67, seed=8)
    tb, ts, tm = (torch.from_numpy(a).to(dev) for a in (base, sim, bg))
    out = torch.empty((3, 17, 67, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for style in STYLE_CODES.values():
            display.compose(tb, ts, tm, style=style, normalize=True, overlay_ratio=RATIO, colormap=table)
        display.compose(tb, ts, tm, style=display.HEAT, normalize=True, overlay_ratio=RATIO, colormap=table, dtype=torch.uint8,
                        out=out)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    same(out, ref.compose(base, sim, bg, style=ref.HEAT, normalize=True, ratio=RATIO, table=table.cpu().numpy(), uint8=True),
         "under sync debug")


# ---- the orchestration: a small seeded scene (the one of tests/test_gpu_relevant_cameras.py) ---------------------------
@pytest.fixture(scope="module")
def scene(dev):
    from tests.test_gpu_relevant_cameras import _cameras, _scene
    cams = _cameras(dev)
    return _scene(dev), [cams[0], cams[2], cams[3]]  # the whole object, a sliver, the object behind the camera


@pytest.mark.parametrize("mode", ["image", "depth", "alpha"])
def test_view_frame_equals_the_restatement_of_its_parts(dev, scene, mode):
    from goi_hyperplane_amd import display
    from goi_hyperplane_amd.semantic import view_frame
    (pc, mlp, lut, score_fn), cams = scene
    table = torch.from_numpy(table_of(256)).to(dev)
    bgc = torch.zeros(3, device=dev)
    for style in STYLE_CODES.values():
        for dtype, u8 in ((torch.float32, False), (torch.uint8, True)):
            frame, parts = view_frame(cams[0], pc, mlp, lut, score_fn, 0.5, bgc, mode=mode, style=style, overlay_ratio=RATIO,
                                      dtype=dtype, colormap=table, return_parts=True)
            base = parts["base"].cpu().numpy()
            assert base.shape[0] == (3 if mode == "image" else 1) and frame.shape == base.shape[1:] + (3,)
            sim = None if parts["sim"] is None else parts["sim"].cpu().numpy()
            bg = None if parts["bg_mask"] is None else parts["bg_mask"].cpu().numpy().astype(bool)
            if style != display.NONE:
                assert bg.any() and not bg.all() and np.array_equal(bg, sim == 0)  # the object and its surroundings
            want = ref.compose(base, sim, bg, style=style, normalize=mode == "depth", ratio=RATIO, table=table.cpu().numpy(),
                               uint8=u8)
            same(frame, want, (mode, ref.STYLE_NAMES[style], u8))


def test_view_frame_decode_is_compute_similarity(dev, scene):
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import compute_similarity, view_frame
    (pc, mlp, lut, score_fn), cams = scene
    bgc = torch.zeros(3, device=dev)
    _, parts = view_frame(cams[0], pc, mlp, lut, score_fn, 0.5, bgc, style="binary", return_parts=True)
    out = render_gui(cams[0], pc, bgc)
    m = torch.zeros(parts["sim"].numel(), dtype=torch.bool, device=dev)
    sim = compute_similarity(out["semantics"], mlp, lut, score_fn, 0.5, out_bg_mask=m)
    assert torch.equal(sim, parts["sim"]) and torch.equal(m, parts["bg_mask"].bool())
    assert torch.equal(out["image"], parts["base"])


@pytest.mark.parametrize("mode,style", [("image", "heat"), ("depth", "heat"), ("image", "whiten"), ("alpha", "none")])
def test_video_frames_equals_view_frame_per_camera(dev, scene, mode, style):
    from goi_hyperplane_amd.semantic import video_frames, view_frame
    (pc, mlp, lut, score_fn), cams = scene
    table = torch.from_numpy(table_of(256)).to(dev)
    bgc = torch.zeros(3, device=dev)
    for dtype in (torch.uint8, torch.float32):
        frames = video_frames(cams, pc, mlp, lut, score_fn, 0.5, bgc, mode=mode, style=style, overlay_ratio=RATIO, dtype=dtype,
                              colormap=table)
        assert frames.shape == (3, 120, 160, 3) and frames.dtype == dtype
        singles = [view_frame(c, pc, mlp, lut, score_fn, 0.5, bgc, mode=mode, style=style, overlay_ratio=RATIO, dtype=dtype,
                              colormap=table) for c in cams]
        for v in range(3):
            same(frames[v], singles[v].cpu().numpy(), (mode, style, v, dtype))
    assert not torch.equal(frames[0], frames[2])
