"""A per-Gaussian selection rendered IN PLACE (render(..., gaussian_mask=m, in_place=True); goi_raster_forward, keep / invert;
DESIGN.md 4.18) against the yardstick: the index-select path render(..., gaussian_mask=m), which restates the reference's
gui/gs_renderer.py:315-321 and is untouched by the selection.

  1. forward: the four maps and num_rendered equal the index-select frame's bit for bit, radii[m] are the subset's radii and
     radii[~m] are 0 -- with the exact forward, the speculative forward, a forced capacity that overflows and is redone, and
     both bindings;
  2. backward: every parameter's .grad and viewspace_points.grad equal the index-select path's as whole P-long tensors (autograd
     scatters those into zeros: the unselected rows are exactly zero), on the full, the semantics-only and the SH-frozen
     backward, and two runs give the same bits;
  3. an in-place frame of the speculative inference forward never synchronises the host;
  4. the geometry cache keys the selection: A, B, none, A again -- each frame equals its uncached frame, the second A is a hit,
     a version bump of A's tensor a miss;
  5. view_frame / video_frames / group_points give the same with in_place, and the P-long outputs feed
     densify.add_densification_stats.

A frame with NONE kept has no index-select counterpart to compare with (the subset is empty: the operator returns zero-filled
maps for P = 0, rasterize_points.cu:84-85): it is checked against what it must be -- the background, alpha 0, num_rendered 0,
radii 0, and gradients that are zero everywhere.
"""
from __future__ import annotations

import types

import pytest
import torch

from goi_hyperplane_amd.scene import make_camera, make_scene

pytestmark = pytest.mark.gpu

MAPS = ("render", "semantics", "depth", "alpha")
# (P, W, H, S, SH degree, precomputed colours + covariances): P = 1000 is four workgroups of the preprocess kernel, the last one
# partial; 70 x 50 is no multiple of the 16-pixel tile
CONFIGS = {
    "p1000_70x50_s16_sh3": (1000, 70, 50, 16, 3, False),
    "p1000_128x96_s10_sh1": (1000, 128, 96, 10, 1, False),
    "p257_128x96_s16_sh3": (257, 128, 96, 16, 3, False),
    "p257_70x50_s10_sh1": (257, 70, 50, 10, 1, False),
    "p1000_70x50_s16_precomp": (1000, 70, 50, 16, 3, True),
}
PARAMS = ("_xyz", "_scaling", "_rotation", "_opacity", "_features", "_semantics")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _C
    _C.set_binding("compiled")  # fails loudly if lib/_goi_C.so has not been built
    return torch.device("cuda:0")


def _default_modes():
    from goi_hyperplane_amd import _C, rasterizer
    _C.poll_counts(wait=True)
    _C.set_binding("compiled")
    _C.set_forward_mode(speculative=True, headroom=2.0, capacity=None, on_overflow="warn", max_ahead=64,
                        inference_speculative=False, min_history=3)
    rasterizer.set_geometry_cache(0)


@pytest.fixture(autouse=True)
def _restore():
    yield
    _default_modes()


def masks_of(P, dev):
    """name -> (mask handed to render, mask_invert, the Gaussians that are rendered)"""
    g = torch.Generator(device=dev).manual_seed(11)
    half = torch.rand(P, device=dev, generator=g) < 0.5
    ones, zeros = torch.ones(P, dtype=torch.bool, device=dev), torch.zeros(P, dtype=torch.bool, device=dev)
    last_dropped, last_kept = ones.clone(), zeros.clone()
    last_dropped[-1], last_kept[-1] = False, True
    out = {"half": (half, False, half), "complement": (half, True, ~half), "all": (ones, False, ones),
           "none": (zeros, False, zeros), "last_dropped": (last_dropped, False, last_dropped),
           "last_kept": (last_kept, False, last_kept)}
    if P >= 512:  # a whole workgroup of the preprocess kernel with nothing to do
        wg = ones.clone()
        wg[256:512] = False
        out["workgroup_dropped"] = (wg, False, wg)
    return out


_SCENES = {}


def scene_of(name, dev):
    """(pc, camera, background, render keywords, extra leaf or None, masks): built once per configuration"""
    if name not in _SCENES:
        from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera
        P, W, H, S, D, precomp = CONFIGS[name]
        sc = make_scene(P, S=S, sh_degree=D, seed=7, log_scale_mean=-2.3)
        pc = GaussianSet.from_scene(sc, dev)
        cam = TorchCamera(make_camera(W, H, yaw=0.15, pitch=-0.05), dev)
        bg = torch.tensor([0.2, 0.5, 0.1], device=dev)
        kw, colors = dict(pipe=PipelineParams()), None
        if precomp:
            g = torch.Generator(device=dev).manual_seed(5)
            colors = torch.rand((P, 3), device=dev, generator=g)
            kw = dict(pipe=PipelineParams(compute_cov3D_python=True), override_color=colors)
        _SCENES[name] = (pc, cam, bg, kw, colors, masks_of(P, dev))
    return _SCENES[name]


def frame(cam, pc, bg, kw, mask, in_place, invert=False):
    """One frame and its count, read BEFORE the outputs are looked at (an overflowed speculative frame is redone there)."""
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.render import render
    out = render(cam, pc, kw["pipe"], bg, override_color=kw.get("override_color"), gaussian_mask=mask, in_place=in_place,
                 mask_invert=invert)
    return out, int(rasterizer.last_num_rendered())


_YARDSTICK = {}


def yardstick(name, dev):
    """mask name -> (maps, num_rendered, radii of the subset): the index-select path, exact forward, once per configuration"""
    if name not in _YARDSTICK:
        from goi_hyperplane_amd import _C
        pc, cam, bg, kw, _colors, masks = scene_of(name, dev)
        _C.set_forward_mode(speculative=False)
        res = {}
        with torch.no_grad():
            for mname, (_m, _inv, eff) in masks.items():
                if mname == "none":
                    continue
                out, n = frame(cam, pc, bg, kw, eff, in_place=False)
                res[mname] = ({k: out[k].clone() for k in MAPS}, n, out["radii"].clone())
        _YARDSTICK[name] = res
    return _YARDSTICK[name]


def check_empty_frame(out, n, bg, S, P):
    H, W = out["alpha"].shape[-2:]
    assert n == 0
    assert torch.equal(out["render"], bg.reshape(3, 1, 1).expand(3, H, W))
    assert tuple(out["semantics"].shape) == (S, H, W) and not out["semantics"].any()
    assert not out["alpha"].any() and not out["depth"].any()
    assert tuple(out["radii"].shape) == (P,) and not out["radii"].any()


# ---- 1. forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
@pytest.mark.parametrize("mode", ["exact", "speculative", "overflow"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_equals_the_index_select_frame(dev, name, mode, binding):
    from goi_hyperplane_amd import _C
    pc, cam, bg, kw, _colors, masks = scene_of(name, dev)
    want = yardstick(name, dev)
    P, S = CONFIGS[name][0], CONFIGS[name][3]
    _C.set_binding(binding)
    assert _C.binding() == binding
    before = dict(_C.SPECULATION_STATS)
    with torch.no_grad():
        for mname, (m, inv, eff) in masks.items():
            n_want = 0 if mname == "none" else want[mname][1]
            if mode == "exact":
                _C.set_forward_mode(speculative=False, capacity=None)
            elif mode == "speculative":
                _C.set_forward_mode(speculative=True, capacity=2 * n_want + 1000)
            else:  # a capacity the frame cannot fit: truncated, then redone when the count is read
                _C.set_forward_mode(speculative=True, capacity=max(1, n_want // 3))
            sel = m.to(torch.uint8) * 255 if mname == "last_dropped" else m  # (any non-zero byte selects)
            out, n = frame(cam, pc, bg, kw, sel, in_place=True, invert=inv)
            assert tuple(out["radii"].shape) == (P,) and tuple(out["visibility_filter"].shape) == (P,)
            assert tuple(out["viewspace_points"].shape) == (P, 3)
            if mname == "none":
                check_empty_frame(out, n, bg, S, P)
                continue
            maps, n0, radii0 = want[mname]
            assert n == n0, (mname, n, n0)
            for k in MAPS:
                assert torch.equal(out[k], maps[k]), (mname, k)
            assert torch.equal(out["radii"][eff], radii0), mname
            assert not out["radii"][~eff].any(), mname
            assert torch.equal(out["visibility_filter"], out["radii"] > 0)
    after = _C.SPECULATION_STATS
    if mode == "exact":
        assert after["speculative_frames"] == before["speculative_frames"]
    else:
        assert after["speculative_frames"] == before["speculative_frames"] + len(masks)
    if mode == "overflow":
        assert after["redone"] > before["redone"] and after["redone"] - before["redone"] == after["overflows"] - before["overflows"]


# ---- 2. backward --------------------------------------------------------------------------------------------------------
def _weights(name, dev):
    _P, W, H, S, _D, _pre = CONFIGS[name]
    g = torch.Generator(device=dev).manual_seed(2)
    return {k: torch.randn(s, device=dev, generator=g) for k, s in (("render", (3, H, W)), ("semantics", (S, H, W)),
                                                                    ("depth", (1, H, W)), ("alpha", (1, H, W)))}


def _step(name, dev, mask, in_place, invert, trainable):
    """forward + backward of a loss over all four maps -> ({leaf name: grad or None}, viewspace gradient, backward kernel)"""
    from goi_hyperplane_amd import rasterizer
    pc, cam, bg, kw, colors, _masks = scene_of(name, dev)
    leaves = dict(pc.named_parameters())
    if colors is not None:
        leaves["override_color"] = colors
    for n, p in leaves.items():
        p.requires_grad_(n in trainable)
        p.grad = None
    try:
        out, _n = frame(cam, pc, bg, kw, mask, in_place, invert)
        w = _weights(name, dev)
        sum((out[k] * w[k]).sum() for k in MAPS).backward()
        grads = {n: (None if p.grad is None else p.grad.clone()) for n, p in leaves.items()}
        return grads, out["viewspace_points"].grad.clone(), rasterizer.last_backward_kernel()
    finally:
        for p in leaves.values():
            p.requires_grad_(True)
            p.grad = None


TRAINABLE = {"full": PARAMS + ("override_color",), "semantics": ("_semantics",),
             "full_no_dsh": ("_xyz", "_scaling", "_rotation", "_opacity", "_semantics")}


# (precomputed colours have no SH operand to freeze: no "full_no_dsh" case for that configuration)
@pytest.mark.parametrize("name,kernel", [(n, k) for n in CONFIGS for k in TRAINABLE if not (k == "full_no_dsh" and CONFIGS[n][5])])
def test_backward_equals_the_index_select_path(dev, name, kernel):
    P = CONFIGS[name][0]
    masks = scene_of(name, dev)[5]
    trainable = TRAINABLE[kernel]
    for mname, (m, inv, eff) in masks.items():
        got, got_vs, used = _step(name, dev, m, True, inv, trainable)
        again, again_vs, _ = _step(name, dev, m, True, inv, trainable)
        assert used == kernel, (mname, used)
        assert tuple(got_vs.shape) == (P, 3) and torch.equal(got_vs, again_vs)
        for n in got:
            assert (got[n] is None) == (again[n] is None) and (got[n] is None or torch.equal(got[n], again[n])), (mname, n)
        if mname == "none":  # (no index-select counterpart: see the module docstring)
            assert not got_vs.any()
            for n, g in got.items():
                assert g is None or not g.any(), n
            continue
        want, want_vs, used0 = _step(name, dev, eff, False, False, trainable)
        assert used0 == kernel
        assert torch.equal(got_vs, want_vs), mname
        for n in want:
            assert (got[n] is None) == (want[n] is None), (mname, n)
            if want[n] is not None:
                assert got[n].shape[0] == P and torch.equal(got[n], want[n]), (mname, n)
                assert not got[n][~eff].any(), (mname, n)
        assert any(g is not None and g.any() for g in got.values()) or not eff.any() or mname == "last_kept", mname


# ---- 3. no host synchronisation -----------------------------------------------------------------------------------------
def test_in_place_frame_never_synchronises(dev):
    from goi_hyperplane_amd import _C, rasterizer
    from goi_hyperplane_amd.render import render
    name = "p1000_128x96_s10_sh1"
    pc, cam, bg, kw, _colors, masks = scene_of(name, dev)
    m = masks["half"][0]
    want = yardstick(name, dev)["half"][0]
    _C.set_forward_mode(speculative=True, capacity=None, inference_speculative=True, min_history=1)
    with torch.no_grad():
        render(cam, pc, kw["pipe"], bg, gaussian_mask=m, in_place=True)  # warm-up: teaches the capacity policy
        int(rasterizer.last_num_rendered())
        torch.cuda.synchronize()
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = render(cam, pc, kw["pipe"], bg, gaussian_mask=m, in_place=True)
            inv = render(cam, pc, kw["pipe"], bg, gaussian_mask=m, in_place=True, mask_invert=True)
            n = rasterizer.last_num_rendered()
            with pytest.raises(RuntimeError):  # the index-select path's nonzero is what the selection saves
                render(cam, pc, kw["pipe"], bg, gaussian_mask=m)
        finally:
            torch.cuda.set_sync_debug_mode(before)
    assert isinstance(n, _C.LazyCount)  # (the frames were speculative: no read-back either)
    for k in MAPS:
        assert torch.equal(out[k], want[k]), k
        assert torch.equal(inv[k], yardstick(name, dev)["complement"][0][k]), k


# ---- 4. geometry cache --------------------------------------------------------------------------------------------------
def test_geometry_cache_keys_the_selection(dev):
    from goi_hyperplane_amd import rasterizer
    name = "p1000_70x50_s16_sh3"
    pc, cam, bg, kw, _colors, masks = scene_of(name, dev)
    want = yardstick(name, dev)
    A, B = masks["half"][0].clone(), masks["workgroup_dropped"][0].clone()
    for n, p in pc.named_parameters():
        p.requires_grad_(n == "_semantics")
    try:
        rasterizer.set_geometry_cache(1 << 30)
        seq, st0 = [], rasterizer.geometry_cache_stats()
        for sel, key in ((A, "half"), (B, "workgroup_dropped"), (None, "all"), (A, "half")):
            out, n = frame(cam, pc, bg, kw, sel, in_place=True)
            st = rasterizer.geometry_cache_stats()
            seq.append((st["hits"] - st0["hits"], st["misses"] - st0["misses"]))
            assert n == want[key][1], key
            for k in MAPS:
                assert torch.equal(out[k].detach(), want[key][0][k]), (key, k)
        assert [s[1] for s in seq] == [1, 2, 3, 3] and [s[0] for s in seq] == [0, 0, 0, 1], seq
        # the second A, a reblend, still trains: its semantic gradient is the index-select path's
        g = torch.Generator(device=dev).manual_seed(2)
        w = torch.randn(out["semantics"].shape, device=dev, generator=g)
        pc._semantics.grad = None
        (out["semantics"] * w).sum().backward()
        cached = pc._semantics.grad.clone()
        rasterizer.set_geometry_cache(0)
        pc._semantics.grad = None
        o2, _ = frame(cam, pc, bg, kw, A, in_place=False)
        (o2["semantics"] * w).sum().backward()
        assert torch.equal(cached, pc._semantics.grad)
        # the same tensor, overwritten in place: another version, a miss -- and the frame of what it holds NOW
        rasterizer.set_geometry_cache(1 << 30)
        frame(cam, pc, bg, kw, A, in_place=True)
        base = rasterizer.geometry_cache_stats()
        A.copy_(B)
        out, n = frame(cam, pc, bg, kw, A, in_place=True)
        st = rasterizer.geometry_cache_stats()
        assert (st["hits"], st["misses"]) == (base["hits"], base["misses"] + 1)
        for k in MAPS:
            assert torch.equal(out[k].detach(), want["workgroup_dropped"][0][k]), k
        # the invert flag is part of the key as well
        out, n = frame(cam, pc, bg, kw, masks["half"][0], in_place=True, invert=True)
        for k in MAPS:
            assert torch.equal(out[k].detach(), want["complement"][0][k]), k
    finally:
        rasterizer.set_geometry_cache(0)
        for p in pc.parameters():
            p.requires_grad_(True)
            p.grad = None


# ---- 5. callers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs(dev):
    from tests.test_gpu_group_points import _scene
    return _scene(dev)


@pytest.mark.parametrize("style", ["heat", "none"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_view_frame_and_video_frames_in_place(dev, blobs, style, dtype):
    from goi_hyperplane_amd.semantic import video_frames, view_frame
    pc, _kind, mlp, lut, score_fn, cam = blobs
    P = pc.get_xyz.shape[0]
    g = torch.Generator(device=dev).manual_seed(4)
    m = torch.rand(P, device=dev, generator=g) < 0.5
    bg = torch.zeros(3, device=dev)
    for inv in (False, True):
        a = view_frame(cam, pc, mlp, lut, score_fn, 0.5, bg, style=style, gaussian_mask=m, dtype=dtype, mask_invert=inv)
        b = view_frame(cam, pc, mlp, lut, score_fn, 0.5, bg, style=style, gaussian_mask=m, dtype=dtype, mask_invert=inv,
                       in_place=True)
        assert a.dtype == dtype and torch.equal(a, b)
        if inv:  # mask_invert on the index-select path is the frame of ~m
            c = view_frame(cam, pc, mlp, lut, score_fn, 0.5, bg, style=style, gaussian_mask=~m, dtype=dtype)
            assert torch.equal(a, c)
        va = video_frames([cam, cam], pc, mlp, lut, score_fn, 0.5, bg, style=style, gaussian_mask=m, dtype=dtype, mask_invert=inv)
        vb = video_frames([cam, cam], pc, mlp, lut, score_fn, 0.5, bg, style=style, gaussian_mask=m, dtype=dtype, mask_invert=inv,
                          in_place=True)
        assert va.dtype == dtype and torch.equal(va, vb)
    assert float(b.float().std()) > 0  # (a frame with something in it)


def test_group_points_in_place(dev, blobs):
    from goi_hyperplane_amd.semantic import group_points, select_gaussians
    from tests.test_gpu_group_points import _res_mask_of
    pc, kind, mlp, lut, score_fn, cam = blobs
    bg = torch.zeros(3, device=dev)
    selected = select_gaussians(pc, mlp, lut, score_fn)
    res = _res_mask_of(pc, kind == 0, cam, bg, mlp, lut, score_fn)
    shown = kind != 1  # blob B is hidden from the renders
    a = group_points(pc, selected, cam, bg, mlp, lut, score_fn, res, gaussian_mask=shown)
    b = group_points(pc, selected, cam, bg, mlp, lut, score_fn, res, gaussian_mask=shown, in_place=True)
    c = group_points(pc, selected, cam, bg, mlp, lut, score_fn, res, gaussian_mask=~shown, in_place=True, mask_invert=True)
    assert a.dtype == torch.bool and a.any() and torch.equal(a, b) and torch.equal(a, c)
    assert pc._semantics_masks is None


def test_in_place_outputs_feed_the_densification_statistics(dev):
    from goi_hyperplane_amd import densify
    name = "p1000_70x50_s16_sh3"
    pc, cam, bg, kw, _colors, masks = scene_of(name, dev)
    P = CONFIGS[name][0]
    m = masks["half"][0]
    stats = lambda: types.SimpleNamespace(xyz_gradient_accum=torch.zeros((P, 1), device=dev),  # noqa: E731
                                          denom=torch.zeros((P, 1), device=dev))
    for p in pc.parameters():
        p.grad = None
    out, _ = frame(cam, pc, bg, kw, m, in_place=True)
    out["render"].sum().backward()
    g = stats()
    densify.add_densification_stats(g, out["viewspace_points"], out["visibility_filter"])
    vis = out["visibility_filter"]
    assert vis.any() and not vis[~m].any()
    assert torch.equal(g.denom.reshape(-1), vis.float())
    # (the norm of two floats: two products, a sum and a square root, each within half an ulp, fused or not -- 8 ulp is generous)
    want = out["viewspace_points"].grad[:, :2].norm(dim=-1, keepdim=True) * vis[:, None]
    assert torch.allclose(g.xyz_gradient_accum, want, rtol=8 * 2.0 ** -24, atol=0)
    # the index-select frame's filter is K-long: not something the statistics of the full model can take
    sub, _ = frame(cam, pc, bg, kw, m, in_place=False)
    sub["render"].sum().backward()
    assert sub["visibility_filter"].shape[0] == int(m.sum()) < P
    with pytest.raises(ValueError):
        densify.add_densification_stats(stats(), sub["viewspace_points"], sub["visibility_filter"])
    for p in pc.parameters():
        p.grad = None
