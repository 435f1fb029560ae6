"""goi_hyperplane_amd.edit on the GPU (csrc/edit.hip): the rigid edit of a selection, in place.

  1. every tensor the edit writes equals the numpy float32 restatement (tests/edit_reference.py) bit for bit, at every wave
     boundary (P = 0, 1, 63, 64, 65, 129, 4099), for every stored SH width (M = 1, 4, 9, 16) and selection shape; unselected rows
     and untouched tensors keep their bits;
  2. the Adam first moments of xyz / rotation / f_rest turn with their parameters; exp_avg_sq, step and the other groups keep
     their bits; moments=False leaves the whole state alone;
  3. selection_bounds: count, lo, hi exact, the centroid within one fp32 ulp of the float64 mean, the empty selection; a derived
     pivot equals the same pivot handed over as a device tensor, and the call never synchronises;
  4. the picture is invariant: transform every Gaussian and the camera, render both;
  5. a transformed half rendered in place equals the model in which only that half exists;
  6. the geometry cache never reblends a camera's geometry after an edit."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch
from torch import nn

from goi_hyperplane_amd import edit
from goi_hyperplane_amd.scene import make_camera, make_scene
from tests import densify_reference as dref
from tests import edit_reference as ref

pytestmark = pytest.mark.gpu

ROT, T, PIVOT = ref.random_rotation(11), (0.3, -0.2, 0.1), (0.1, 0.2, -0.1)
EDITED = ("_xyz", "_rotation", "_scaling", "_features_rest")
MAPS = ("render", "semantics", "depth", "alpha")
GATE = 1e-4  # the project's forward gate (smoke(), tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def snapshot(g):
    """every tensor of the model and its optimizer state, on the host"""
    out = {attr: getattr(g, attr).detach().cpu().numpy().copy() for _, attr in dref.PARAMS}
    for name in dref.STATS:
        out[name] = getattr(g, name).cpu().numpy().copy()
    if g.optimizer is not None:
        for grp in g.optimizer.param_groups:
            st = g.optimizer.state.get(grp["params"][0], None) or {}
            for k, v in st.items():
                out[f"{grp['name']}.{k}"] = v.detach().cpu().numpy().copy() if torch.is_tensor(v) else np.asarray(v)
    return out


def selections(P, dev):
    """name -> (selection handed over, invert, the rows that are edited)"""
    g = torch.Generator().manual_seed(P)
    half = (torch.rand(P, generator=g) < 0.5).to(dev)
    zeros = torch.zeros(P, dtype=torch.bool, device=dev)

    def one(i):
        m = zeros.clone()
        if 0 <= i < P:
            m[i] = True
        return m

    base = {"none": zeros, "all": ~zeros, "half": half, "lane0": one(64 if P > 64 else 0), "lane63": one(127 if P > 127 else 63),
            "last": one(P - 1)}
    out = {"no_selection": (None, False, ~zeros)}
    for name, m in base.items():
        out[name] = (m, False, m)
        out[name + "_inverted"] = (m, True, ~m)
    out["half_uint8"] = (half.to(torch.uint8) * 255, False, half)  # any non-zero byte selects
    return out


def expected(before, eff, **kw):
    """the restatement's edit of a snapshot: {key of the snapshot: array}"""
    arrays = {k: before[k] for k in EDITED}
    for name, attr, key in ref.MOMENTS:
        if f"{name}.exp_avg" in before:
            arrays[key] = before[f"{name}.exp_avg"]
    out = ref.transform(arrays, eff, ref.constants(**kw))
    want = dict(before)
    want.update({k: out[k] for k in EDITED})
    for name, attr, key in ref.MOMENTS:
        if key in out:
            want[f"{name}.exp_avg"] = out[key]
    return want


def assert_model_is(g, want, what):
    got = snapshot(g)
    assert set(got) == set(want), what
    for k in want:
        assert same_bits(got[k], want[k]), (what, k)


# ---- 1. bit-equality with the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 4, 9, 16])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 129, 4099])
def test_edit_equals_the_restatement_bit_for_bit(dev, P, M):
    kw = dict(rotation=ROT, translation=T, scale=1.3, pivot=PIVOT)
    for name, (sel, inv, eff) in selections(P, dev).items():
        g = dref.make_model(P, dev, seed=P + M, M=M, S=4, optimizer="adam" if P else None)
        before = snapshot(g)
        edit.transform(g, sel, invert=inv, **kw)
        want = expected(before, eff.cpu().numpy(), **kw)
        assert_model_is(g, want, name)
        if P and eff.any() and name in ("all", "half", "last"):
            assert not same_bits(want["_features_rest"], before["_features_rest"]) or M == 1
            assert not same_bits(want["_xyz"], before["_xyz"])


@pytest.mark.parametrize("case", ["rotate", "rotate_quaternion", "scale", "translate", "scale_translate", "rotate_about_origin"])
def test_every_kind_of_edit_and_two_runs(dev, case):
    P, M = 4099, 16
    q = edit._matrix_to_quat(ROT)
    kw = {"rotate": dict(rotation=ROT, pivot=PIVOT), "rotate_quaternion": dict(rotation=3.0 * q, pivot=PIVOT),
          "scale": dict(scale=0.5, pivot=PIVOT), "translate": dict(translation=T, pivot=PIVOT),
          "scale_translate": dict(scale=2.0, translation=T, pivot=PIVOT), "rotate_about_origin": dict(rotation=ROT, pivot="origin")}[case]
    sel, _inv, eff = selections(P, dev)["half"]
    runs = []
    for _ in range(2):
        g = dref.make_model(P, dev, seed=3, M=M, S=4, optimizer="adam")
        before = snapshot(g)
        edit.transform(g, sel, **kw)
        runs.append(snapshot(g))
    ref_kw = dict(kw, pivot=(0.0, 0.0, 0.0) if kw["pivot"] == "origin" else kw["pivot"])
    want = expected(before, eff.cpu().numpy(), **ref_kw)
    for k in want:
        assert same_bits(runs[0][k], want[k]), k
        assert same_bits(runs[0][k], runs[1][k]), k
    if case == "rotate_quaternion":  # the quaternion (of any length) is the matrix, up to the rounding of the constants
        by_matrix = expected(before, eff.cpu().numpy(), rotation=ROT, pivot=PIVOT)
        assert np.abs(want["_xyz"] - by_matrix["_xyz"]).max() <= 1e-5
    touched = {k for k in want if not same_bits(want[k], before[k])}
    turned = {"_xyz", "_rotation", "_features_rest", "xyz.exp_avg", "rotation.exp_avg", "f_rest.exp_avg"}
    assert touched == {"scale": {"_xyz", "_scaling"}, "translate": {"_xyz"}, "scale_translate": {"_xyz", "_scaling"}}.get(case, turned)


def test_move_is_the_reference_s_indexed_add(dev):
    P = 4099
    for name in ("half", "last", "none", "all"):
        sel, _inv, eff = selections(P, dev)[name]
        g = dref.make_model(P, dev, seed=5, M=16, S=4, optimizer="adam")
        before = snapshot(g)
        d = torch.tensor([0.1, 0.0, -0.3]) * 0.1
        want = g._xyz.detach().clone()
        want[eff] += d.to(dev)  # gui/main_edit.py:1544
        edit.move(g, sel, d)
        assert torch.equal(g._xyz.detach(), want) and same_bits(g._xyz.detach().cpu().numpy(), want.cpu().numpy())
        after = snapshot(g)
        for k in before:
            assert k == "_xyz" or same_bits(after[k], before[k]), k


def test_rows_that_are_only_four_byte_aligned(dev):
    """_features_rest rows are 180 bytes: a model whose tensors start one float into their storage (a view)"""
    P, M = 200, 16
    g = dref.make_model(P, dev, seed=9, M=M, S=4, optimizer=None)
    for attr in EDITED:
        t = getattr(g, attr).detach()
        store = torch.zeros(t.numel() + 1, device=dev)
        view = store[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        setattr(g, attr, nn.Parameter(view))
    before = snapshot(g)
    sel, _inv, eff = selections(P, dev)["half"]
    kw = dict(rotation=ROT, translation=T, scale=0.8, pivot=PIVOT)
    edit.transform(g, sel, **kw)
    assert_model_is(g, expected(before, eff.cpu().numpy(), **kw), "offset views")


# ---- 2. the Adam state ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer,steps", [("adam", 2), ("adam", 0), ("fused", 2), ("fused", 0), (None, 0), ("partial", 2)])
def test_first_moments_turn_and_everything_else_keeps_its_bits(dev, optimizer, steps):
    P, M = 1000, 16
    sel, _inv, eff = selections(P, dev)["half"]
    kw = dict(rotation=ROT, translation=T, scale=1.5, pivot=PIVOT)
    g = dref.make_model(P, dev, seed=21, M=M, S=4, optimizer=optimizer, steps=steps)
    before = snapshot(g)
    edit.transform(g, sel, **kw)
    want = expected(before, eff.cpu().numpy(), **kw)
    assert_model_is(g, want, optimizer)
    moved = {k for k in want if k.endswith(".exp_avg") and not same_bits(want[k], before[k])}
    if optimizer in ("adam", "fused") and steps:
        assert moved == {"xyz.exp_avg", "rotation.exp_avg", "f_rest.exp_avg"}
        assert {"xyz.exp_avg_sq", "xyz.step", "scaling.exp_avg", "f_dc.exp_avg", "opacity.exp_avg"} <= set(want)
    elif optimizer == "partial":
        assert moved == {"f_rest.exp_avg"} and "f_dc.exp_avg" in want and "xyz.exp_avg" not in want
    else:
        assert not moved and not any(k.endswith(".exp_avg") for k in want)
    # the optimizer still steps on the edited parameters (the state is keyed by the same Parameter objects)
    if optimizer is not None:
        for grp in g.optimizer.param_groups:
            p = grp["params"][0]
            p.grad = torch.ones_like(p)
        g.optimizer.step()
    # moments=False: the parameters move, the state does not
    g = dref.make_model(P, dev, seed=21, M=M, S=4, optimizer=optimizer, steps=steps)
    edit.transform(g, sel, moments=False, **kw)
    after = snapshot(g)
    for k in before:
        if "." in k:
            assert same_bits(after[k], before[k]), k
        else:
            assert same_bits(after[k], want[k]), k


# ---- 3. bounds and the derived pivot ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 1, 255, 257, 4099, 300001])  # 300001 rows: more than the 1024 workgroups own one row each
def test_selection_bounds(dev, P):
    g = torch.Generator().manual_seed(P)
    xyz = (torch.randn(P, 3, generator=g) * torch.tensor([3.0, 0.5, 10.0]) + torch.tensor([100.0, -0.01, 3.0])).to(dev)
    half = (torch.rand(P, generator=g) < 0.5).to(dev)
    cases = [(None, False, torch.ones(P, dtype=torch.bool, device=dev)), (half, False, half), (half, True, ~half),
             (half.to(torch.uint8), False, half), (torch.zeros(P, dtype=torch.bool, device=dev), False, torch.zeros_like(half))]
    for sel, inv, eff in cases:
        b = edit.selection_bounds(xyz, sel, invert=inv)
        again = edit.selection_bounds(xyz, sel, invert=inv)
        assert b["count"].dtype == torch.int32 and tuple(b["count"].shape) == (1,) and b["count"].device == xyz.device
        rows = xyz[eff].cpu().numpy()
        n = rows.shape[0]
        assert int(b["count"]) == n
        for k in ("lo", "hi", "centroid", "center"):
            assert b[k].dtype == torch.float32 and tuple(b[k].shape) == (3,) and b[k].device == xyz.device
            assert same_bits(b[k].cpu().numpy(), again[k].cpu().numpy()), k  # the same bits on every run
        lo, hi = b["lo"].cpu().numpy(), b["hi"].cpu().numpy()
        cen, mid = b["centroid"].cpu().numpy(), b["center"].cpu().numpy()
        if n == 0:
            assert (lo == np.inf).all() and (hi == -np.inf).all() and not cen.any() and not mid.any()
            continue
        assert same_bits(lo, rows.min(axis=0)) and same_bits(hi, rows.max(axis=0))
        assert same_bits(mid, np.float32(0.5) * lo + np.float32(0.5) * hi)
        mean = rows.astype(np.float64).mean(axis=0)
        assert (np.abs(cen.astype(np.float64) - mean) <= np.spacing(np.abs(mean).astype(np.float32))).all(), (cen, mean)


@pytest.mark.parametrize("pivot", ["centroid", "center"])
def test_derived_pivot_equals_the_device_pivot_and_never_synchronises(dev, pivot):
    P, M = 4099, 16
    kw = dict(rotation=ROT, translation=T, scale=1.2)
    for name in ("half", "half_inverted", "none", "no_selection"):
        sel, inv, eff = selections(P, dev)[name]
        a = dref.make_model(P, dev, seed=8, M=M, S=4, optimizer="adam")
        b = dref.make_model(P, dev, seed=8, M=M, S=4, optimizer="adam")
        before = snapshot(a)
        p = edit.selection_bounds(b._xyz.detach(), sel, invert=inv)[pivot].clone()
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            edit.transform(a, sel, invert=inv, pivot=pivot, **kw)
            edit.transform(b, sel, invert=inv, pivot=p, **kw)
            edit.move(b, sel, (0.0, 0.0, 0.0))
            edit.selection_bounds(b._xyz.detach(), sel, invert=inv)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        got = snapshot(a)
        assert_model_is(b, got, name)
        want = expected(before, eff.cpu().numpy(), pivot=p.cpu().numpy(), **kw)  # and both are the restatement at that pivot
        for k in want:
            assert same_bits(got[k], want[k]), (name, k)


# ---- 4. invariance of the picture -------------------------------------------------------------------------------------------
def scene_model(sc, dev, rows=None):
    """A reference-style model (raw parameters) holding the scene `sc` (its rows `rows`)."""
    t = lambda a: torch.tensor(a if rows is None else a[rows], dtype=torch.float32, device=dev).contiguous()  # noqa: E731
    m = dref.Model()
    m._xyz = nn.Parameter(t(sc.means3D))
    m._scaling = nn.Parameter(t(np.log(sc.scales)))
    m._rotation = nn.Parameter(t(sc.rotations))
    m._opacity = nn.Parameter(t(np.log(sc.opacities / (1 - sc.opacities))))
    m._features_dc = nn.Parameter(t(sc.shs[:, :1]))
    m._features_rest = nn.Parameter(t(sc.shs[:, 1:]))
    m._semantics = nn.Parameter(t(sc.semantics))
    return m


def frame(cam, m, dev, **kw):
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    with torch.no_grad():
        out = render(TorchCamera(cam, dev), m, PipelineParams(), torch.tensor([0.1, 0.2, 0.3], device=dev), **kw)
    return {k: out[k].detach().clone() for k in MAPS + ("radii",)}


# The s = 1 cases are scenes 0 and 1.  The scene of the s = 2 case is chosen by the REFERENCE's own error, measured without any of
# the code under test (tests/test_edit_cpu.py::test_the_oracle_s_own_response_to_a_rigid_motion_picks_the_scale_case): the CPU
# oracle, fed the numpy-restated edit of the scene and transform_camera's camera, rotations random_rotation(40 .. 47), s = 1 and 2.
# On scene 1 it stays within 1.1e-5 on all 16 motions.  On scene 0 it jumps by 2.02e-3 (colour), 4.67e-3 (semantics) and
# 1.01e-4 (alpha) at ONE pixel, row 3 column 39, on 2 of the 16: a pixel the oracle marks `fragile` in the untouched frame (a
# discrete decision of the blend within 1e-4 of its threshold, which any perturbation of the inputs can tip).  A scene on which
# the reference itself leaves the gate under a rigid motion cannot carry a gate of 1e-4 with no pixel excluded; scene 1 can.
@pytest.mark.parametrize("seed,scale", [(0, 1.0), (1, 1.0), (1, 2.0)])
def test_the_picture_is_invariant_when_model_and_camera_move_together(dev, seed, scale):
    """Every Gaussian goes through edit.transform on the GPU, the camera through transform_camera; both frames are rendered
    and every pixel of colour, semantics, depth and alpha is compared with the forward gate of 1e-4 (under s = 2 the depth
    after division by 2).  What the gate has to absorb is the fp32 rasterizer's response to a rigid motion of its inputs:
    the CPU oracle alone, fed the float64-transformed scene and camera, moved by at most 1.1e-5 (depth), 2.7e-6 (colour),
    8.2e-6 (semantics) and 2.4e-6 (alpha) with identical radii and instance counts on seeds 0-3 -- an order of magnitude
    inside the gate.

    Measured on an MI355X (colour, semantics, depth, alpha; radii identical in every case): seed 0, s = 1: 1.9e-6, 7.3e-6,
    4.8e-6, 1.2e-6; seed 1, s = 1: 1.8e-6, 6.9e-6, 6.2e-6, 1.2e-6; seed 1, s = 2: 1.5e-6, 6.3e-6, 6.4e-6, 1.3e-6."""
    from goi_hyperplane_amd import _C
    _C.set_forward_mode(speculative=False)
    try:
        sc = make_scene(3000, S=4, seed=seed, log_scale_mean=-2.5)
        cam = make_camera(96, 64, yaw=0.3, pitch=-0.2)
        m = scene_model(sc, dev)
        before = frame(cam, m, dev)
        kw = dict(rotation=ref.random_rotation(40 + seed), translation=T, scale=scale, pivot=PIVOT)
        edit.transform(m, None, **kw)
        after = frame(edit.transform_camera(cam, **kw), m, dev)
    finally:
        _C.set_forward_mode(speculative=True)
    assert float(before["alpha"].max()) > 0.5 and int((before["radii"] > 0).sum()) > 1000  # a frame with something in it
    worst = {}
    for k in MAPS:
        d = ((after[k] / scale if k == "depth" else after[k]) - before[k]).abs().amax(dim=0)
        worst[k] = float(d.max())
        print(f"seed {seed} scale {scale} {k}: max |difference| = {worst[k]:.3e}, pixels at or over the gate: {int((d >= GATE).sum())}")
    print(f"seed {seed} scale {scale} radii that differ: {int((after['radii'] != before['radii']).sum())}")
    for k in MAPS:
        assert worst[k] < GATE, (k, worst)


# ---- 5. part of the model ---------------------------------------------------------------------------------------------------
def test_a_transformed_half_rendered_in_place_is_the_model_of_that_half(dev):
    sc = make_scene(3000, S=4, seed=2, log_scale_mean=-2.5)
    cam = make_camera(96, 64, yaw=0.3, pitch=-0.2)
    sel = torch.rand(3000, generator=torch.Generator().manual_seed(1)) < 0.5
    whole, part = scene_model(sc, dev), scene_model(sc, dev, rows=sel.numpy())
    sel = sel.to(dev)
    kw = dict(rotation=ROT, translation=T, scale=1.1, pivot=PIVOT)
    untouched = frame(cam, whole, dev, gaussian_mask=sel, in_place=True, mask_invert=True)
    edit.transform(whole, sel, **kw)
    edit.transform(part, None, **kw)
    a = frame(cam, whole, dev, gaussian_mask=sel, in_place=True)
    b = frame(cam, part, dev)
    for k in MAPS:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["radii"][sel], b["radii"]) and not a["radii"][~sel].any()
    assert float(b["alpha"].max()) > 0.5
    rest = frame(cam, whole, dev, gaussian_mask=sel, in_place=True, mask_invert=True)  # and the other half has not moved
    for k in MAPS:
        assert torch.equal(rest[k], untouched[k]), k


# ---- 6. the geometry cache --------------------------------------------------------------------------------------------------
def test_the_geometry_cache_never_reblends_a_camera_after_an_edit(dev):
    from goi_hyperplane_amd import _C, rasterizer
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    sc = make_scene(3000, S=4, seed=3, log_scale_mean=-2.5)
    m = scene_model(sc, dev)
    for _, attr in dref.PARAMS:  # the semantic stage: only the features train, so the frames are eligible for the cache
        getattr(m, attr).requires_grad_(attr == "_semantics")
    cam = TorchCamera(make_camera(96, 64, yaw=0.3, pitch=-0.2), dev)
    bg = torch.zeros(3, device=dev)
    shot = lambda: {k: v.detach().clone() for k, v in render(cam, m, PipelineParams(), bg).items() if k in MAPS}  # noqa: E731
    sel = (torch.rand(3000, generator=torch.Generator().manual_seed(4)) < 0.5).to(dev)
    rasterizer.set_geometry_cache(1 << 30)
    try:
        first = shot()
        _C.poll_counts(dev, wait=True)
        s0 = rasterizer.geometry_cache_stats()
        again = shot()
        s1 = rasterizer.geometry_cache_stats()
        assert s1["hits"] == s0["hits"] + 1  # (the camera IS served from the cache while nothing changes)
        versions = {attr: getattr(m, attr)._version for _, attr in dref.PARAMS}
        edit.transform(m, sel, rotation=ROT, translation=T, scale=1.2, pivot="centroid")
        for attr in EDITED:
            assert getattr(m, attr)._version > versions[attr], attr
        for attr in ("_features_dc", "_opacity", "_semantics"):
            assert getattr(m, attr)._version == versions[attr], attr
        cached = shot()
        s2 = rasterizer.geometry_cache_stats()
        assert (s2["hits"], s2["misses"]) == (s1["hits"], s1["misses"] + 1)
        rasterizer.set_geometry_cache(0)
        plain = shot()
        for k in MAPS:
            assert torch.equal(cached[k], plain[k]), k
            assert torch.equal(again[k], first[k]), k
        assert not torch.equal(cached["render"], first["render"])  # the edit did change the picture
        # a translation alone bumps the positions' version as well
        rasterizer.set_geometry_cache(1 << 30)
        shot()
        _C.poll_counts(dev, wait=True)
        v = m._xyz._version
        edit.move(m, sel, (0.05, 0.0, 0.0))
        assert m._xyz._version > v
        moved = shot()
        rasterizer.set_geometry_cache(0)
        plain = shot()
        for k in MAPS:
            assert torch.equal(moved[k], plain[k]), k
    finally:
        rasterizer.set_geometry_cache(0)


def test_moments_versions_grow_too(dev):
    g = dref.make_model(500, dev, seed=1, M=16, S=4, optimizer="adam")
    state = lambda n, k: g.optimizer.state[getattr(g, dref.ATTR[n])][k]  # noqa: E731
    v = {n: (state(n, "exp_avg")._version, state(n, "exp_avg_sq")._version) for n in ("xyz", "rotation", "f_rest", "scaling")}
    edit.transform(g, None, rotation=ROT, scale=2.0, pivot="origin")
    for n in ("xyz", "rotation", "f_rest"):
        assert state(n, "exp_avg")._version > v[n][0] and state(n, "exp_avg_sq")._version == v[n][1], n
    assert state("scaling", "exp_avg")._version == v["scaling"][0]
    assert math.isfinite(float(g._xyz.detach().abs().max()))
