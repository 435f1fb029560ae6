"""goi_hyperplane_amd.pose on the GPU (csrc/pose.hip): the pose gradient of a selection from one backward.

  1. the seven numbers are within gamma(3 P) sum |piece| (float64 unit roundoff: the error of ANY order of the float64 additions)
     of the exact sum of the float32 pieces of tests/pose_reference.py, at every wave boundary, SH width and selection shape: a
     single fp32 rounding that differs in one typical row is outside it;
  2. a gradient that is None is omitted; offset coordinates cancel in d = x - p; two runs, and the same rows through `selection`
     and through `invert` of the complement, give the same 56 bytes;
  3. derived, host and device pivots agree and nothing synchronises; rows that are only 4-byte aligned;
  4. camera_gradient is the negation; the .grad tensors a real backward leaves are consumed as they are;
  5. fit() brings a displaced cluster back towards where the photographs show it."""
from __future__ import annotations

import itertools
import math

import numpy as np
import pytest
import torch
from torch import nn

from goi_hyperplane_amd import edit, pose
from goi_hyperplane_amd.scene import make_camera, make_scene
from tests import densify_reference as dref
from tests import edit_reference as eref
from tests import pose_reference as ref

pytestmark = pytest.mark.gpu

PIVOT = (0.1, 0.2, -0.1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def model(P, dev, seed, M=16, present=pose.GRADS):
    """a seeded model whose .grad tensors are seeded too (those in `present`; the others stay None)"""
    g = dref.make_model(P, dev, seed=seed, M=M, S=4, optimizer=None)
    gen = torch.Generator().manual_seed(seed + 1000)
    for attr in pose.GRADS:
        p = getattr(g, attr)
        grad = torch.randn(p.shape, generator=gen)
        p.grad = grad.to(dev) if attr in present else None
    return g


def host(g):
    arrays = {k: getattr(g, k).detach().cpu().numpy() for k in pose.GRADS}
    grads = {k: None if getattr(g, k).grad is None else getattr(g, k).grad.cpu().numpy() for k in pose.GRADS}
    return arrays, grads


def seven(out):
    """float64 [7] on the host: omega | t | sigma"""
    return np.concatenate([out["rotation"].cpu().numpy(), out["translation"].cpu().numpy(),
                           out["log_scale"].reshape(1).cpu().numpy()])


def assert_gate(out, arrays, grads, eff, pivot, what):
    """the restatement gate: |out - exact sum of the fp32 pieces| <= gamma(3 P) sum |piece| per component, and the count"""
    P = len(eff)
    for k in ("rotation", "translation", "log_scale"):
        assert out[k].dtype == torch.float64 and out[k].device.type == "cuda", k
    assert tuple(out["rotation"].shape) == (3,) and tuple(out["translation"].shape) == (3,) and tuple(out["log_scale"].shape) == ()
    assert out["count"].dtype == torch.int32 and tuple(out["count"].shape) == (1,)
    assert int(out["count"]) == int(eff.sum()), what
    sums, mags = ref.exact_sums(ref.terms(arrays, grads, eff, np.asarray(pivot, dtype=np.float32)))
    got = seven(out)
    assert (np.abs(got - sums) <= ref.bound(P, mags)).all(), (what, got - sums, ref.bound(P, mags))
    return got, sums, mags


def selections(P, dev):
    """name -> (selection handed over, invert, the rows reduced over): the shapes of tests/test_gpu_edit.py"""
    idx = torch.arange(P)
    zeros = torch.zeros(P, dtype=torch.bool)

    def one(i):
        m = zeros.clone()
        if 0 <= i < P:
            m[i] = True
        return m

    base = {"none": zeros, "all": ~zeros, "alternating": idx % 2 == 0, "one_row": one(64 if P > 64 else 0), "last": one(P - 1),
            "empty_wave_next_to_a_full_one": (idx >= 64) & (idx < 128) if P > 64 else idx >= 32}
    out = {"no_selection": (None, False, ~zeros)}
    for name, m in base.items():
        out[name] = (m.to(dev), False, m)
        out[name + "_inverted"] = (m.to(dev), True, ~m)
    out["alternating_uint8"] = ((base["alternating"].to(torch.uint8) * 255).to(dev), False, base["alternating"])
    return out


# ---- 1. the restatement gate -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 4, 9, 16])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 129, 4099])
def test_gradient_is_the_exact_sum_of_the_restated_pieces(dev, P, M):
    g = model(P, dev, seed=P + M, M=M)
    arrays, grads = host(g)
    hit = 0
    for name, (sel, inv, eff) in selections(P, dev).items():
        out = pose.gradient(g, sel, pivot=PIVOT, invert=inv)
        got, sums, mags = assert_gate(out, arrays, grads, eff.numpy(), PIVOT, name)
        if not eff.any():
            assert not got.any(), name  # an empty selection (and P = 0): exact zeros
        else:
            hit += 1
            assert np.all(mags > 0) and np.all(got != 0), name
    assert hit or P == 0


def test_a_single_different_rounding_breaks_the_gate():
    """what the gate can see, without the device: the same pieces with ONE fused multiply-add in ONE row (d_1 g_2 - d_2 g_1 with
    the second product unrounded) leave it, at the largest size of the grid (where the gate is widest)"""
    P = 4099
    rng = np.random.default_rng(0)
    arrays = {"_xyz": rng.normal(size=(P, 3)).astype(np.float32)}
    grads = {"_xyz": rng.normal(size=(P, 3)).astype(np.float32)}
    eff = np.ones(P, bool)
    pieces = ref.terms(arrays, grads, eff, PIVOT)
    sums, mags = ref.exact_sums(pieces)
    d = arrays["_xyz"].astype(np.float64) - np.asarray(PIVOT, np.float32).astype(np.float64)  # (exact: |d| needs < 53 bits)
    gx = grads["_xyz"].astype(np.float64)
    first = (d[:, 1] * gx[:, 2]).astype(np.float32).astype(np.float64)  # the first product rounded, the second one fused
    fused = (first - d[:, 2] * gx[:, 1]).astype(np.float32)
    rows = np.flatnonzero(fused != pieces["omega"][0][:, 0])
    assert len(rows) > P // 10  # (a fused multiply-add differs from two roundings in a good part of the rows)
    delta = np.abs(fused[rows].astype(np.float64) - pieces["omega"][0][rows, 0].astype(np.float64))
    print(f"one different rounding: median {np.median(delta):.2e}, the gate {ref.bound(P, mags)[0]:.2e}")
    assert np.median(delta) > 4 * ref.bound(P, mags)[0]  # (one fp32 ulp of a number near 1 against 3 P float64 roundings of P)


def test_many_rows_per_partial(dev):
    """300001 rows: each of the 1024 per-workgroup partials covers many rows, and every thread more than one"""
    P = 300001
    g = model(P, dev, seed=2, M=16)
    arrays, grads = host(g)
    half = torch.rand(P, generator=torch.Generator().manual_seed(3)) < 0.5
    out = pose.gradient(g, half.to(dev), pivot=PIVOT)
    assert_gate(out, arrays, grads, half.numpy(), PIVOT, "half")
    inv = pose.gradient(g, (~half).to(dev), pivot=PIVOT, invert=True)
    assert seven(inv).tobytes() == seven(out).tobytes()


# ---- 2. optional gradients, cancellation, reproducibility ------------------------------------------------------------------
SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(pose.GRADS, n)]


@pytest.mark.parametrize("present", SUBSETS, ids=["+".join(a.strip("_") for a in s) for s in SUBSETS])
def test_a_gradient_that_is_none_is_omitted(dev, present):
    P, M = 129, 16
    assert len(SUBSETS) == 15
    g = model(P, dev, seed=17, M=M, present=present)
    arrays, grads = host(g)
    sel, inv, eff = selections(P, dev)["alternating"]
    out = pose.gradient(g, sel, pivot=PIVOT)
    got, _sums, _mags = assert_gate(out, arrays, grads, eff.numpy(), PIVOT, present)
    if "_xyz" not in present:
        assert not got[3:6].any()  # nothing else moves the translation
    if "_xyz" not in present and "_scaling" not in present:
        assert got[6] == 0.0
    if not {"_xyz", "_rotation", "_features_rest"} & set(present):
        assert not got[0:3].any()
    # the same through grads=: a dict for torch.autograd.grad users, the .grad tensors ignored
    full = model(P, dev, seed=17, M=M)
    by_dict = pose.gradient(full, sel, pivot=PIVOT, grads={k: getattr(full, k).grad if k in present else None for k in pose.GRADS})
    assert seven(by_dict).tobytes() == got.tobytes()


def test_all_gradients_none_is_refused(dev):
    g = model(129, dev, seed=1, present=())
    with pytest.raises(ValueError, match="run a backward first"):
        pose.gradient(g)
    g = model(129, dev, seed=1, M=1, present=("_features_rest",))  # [P, 0, 3]: there is nothing in it
    with pytest.raises(ValueError, match="run a backward first"):
        pose.gradient(g)


def test_offset_coordinates_cancel_in_d(dev):
    """coordinates near 1000 with the pivot at the centroid: d = x - p is formed first (exact to an ulp of d, not of x g)"""
    P, M = 4099, 16
    g = model(P, dev, seed=23, M=M)
    with torch.no_grad():
        g._xyz += 1000.0
    arrays, grads = host(g)
    sel, inv, eff = selections(P, dev)["alternating"]
    centroid = edit.selection_bounds(g._xyz.detach(), sel)["centroid"].cpu().numpy()
    assert np.all(np.abs(centroid - 1000.0) < 1.0)
    out = pose.gradient(g, sel, pivot="centroid")
    got, sums, mags = assert_gate(out, arrays, grads, eff.numpy(), centroid, "offset")
    assert mags[0] < 1e5  # |d| ~ 1: had the products been formed on x, the magnitudes were a thousand times these


def test_two_runs_and_the_inverted_complement_give_the_same_bytes(dev):
    P = 4099
    for M in (1, 16):
        g = model(P, dev, seed=31, M=M)
        sel = (torch.rand(P, generator=torch.Generator().manual_seed(5)) < 0.5).to(dev)
        a = seven(pose.gradient(g, sel, pivot=PIVOT))
        b = seven(pose.gradient(g, sel, pivot=PIVOT))
        c = seven(pose.gradient(g, ~sel, pivot=PIVOT, invert=True))
        d = seven(pose.gradient(g, sel.to(torch.uint8), pivot=PIVOT))
        assert len(a.tobytes()) == 56 and a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()
        assert a.any()


# ---- 3. pivots, synchronisation, alignment ---------------------------------------------------------------------------------
@pytest.mark.parametrize("pivot", ["centroid", "center"])
def test_derived_pivot_equals_the_device_pivot_and_never_synchronises(dev, pivot):
    P, M = 4099, 16
    g = model(P, dev, seed=8, M=M)
    arrays, grads = host(g)
    for name in ("alternating", "alternating_inverted", "none", "no_selection"):
        sel, inv, eff = selections(P, dev)[name]
        p = edit.selection_bounds(g._xyz.detach(), sel, invert=inv)[pivot].clone()
        p_host = p.cpu().numpy()
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            derived = pose.gradient(g, sel, pivot=pivot, invert=inv)
            device = pose.gradient(g, sel, pivot=p, invert=inv)
            hosted = pose.gradient(g, sel, pivot=p_host, invert=inv)
            origin = pose.gradient(g, sel, pivot="origin", invert=inv)
            camera = pose.camera_gradient(g, pivot=p)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        got, _, _ = assert_gate(derived, arrays, grads, eff.numpy(), p_host, name)
        assert seven(device).tobytes() == got.tobytes() and seven(hosted).tobytes() == got.tobytes(), name
        assert_gate(origin, arrays, grads, eff.numpy(), (0.0, 0.0, 0.0), name)
        assert set(camera) == {"rotation", "translation"}


def test_rows_that_are_only_four_byte_aligned(dev):
    """_features_rest rows are 180 bytes: tensors and gradients that start one float into their storage (views)"""
    P, M = 200, 16
    g = model(P, dev, seed=9, M=M)
    for attr in pose.GRADS:
        t, grad = getattr(g, attr).detach(), getattr(g, attr).grad
        views = []
        for src in (t, grad):
            store = torch.zeros(src.numel() + 1, device=dev)
            view = store[1:].view(src.shape)
            view.copy_(src)
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            views.append(view)
        p = nn.Parameter(views[0])
        p.grad = views[1]
        assert p.grad.data_ptr() % 16 == 4
        setattr(g, attr, p)
    arrays, grads = host(g)
    sel, inv, eff = selections(P, dev)["alternating"]
    assert_gate(pose.gradient(g, sel, pivot=PIVOT), arrays, grads, eff.numpy(), PIVOT, "offset views")


# ---- 4. the camera, and a real backward -------------------------------------------------------------------------------------
def test_camera_gradient_is_the_negated_whole_model_gradient(dev):
    g = model(4099, dev, seed=12, M=16)
    centre = (0.3, -0.2, -5.0)
    for pivot in ("origin", centre, torch.tensor(centre, device=dev)):
        cam = pose.camera_gradient(g, pivot=pivot)
        whole = pose.gradient(g, None, pivot=pivot)
        assert set(cam) == {"rotation", "translation"} and "log_scale" not in cam
        for k in cam:
            assert cam[k].dtype == torch.float64 and torch.equal(cam[k], -whole[k]) and bool(cam[k].abs().sum() > 0), k
    with pytest.raises(ValueError):
        pose.camera_gradient(g, pivot="middle")


def scene_model(sc, dev):
    """A reference-style model (raw parameters) holding the scene `sc`."""
    t = lambda a: nn.Parameter(torch.tensor(a, dtype=torch.float32, device=dev).contiguous())  # noqa: E731
    m = dref.Model()
    m._xyz, m._scaling, m._rotation = t(sc.means3D), t(np.log(sc.scales)), t(sc.rotations)
    m._opacity = t(np.log(sc.opacities / (1 - sc.opacities)))
    m._features_dc, m._features_rest, m._semantics = t(sc.shs[:, :1]), t(sc.shs[:, 1:]), t(sc.semantics)
    return m


def test_the_gradients_a_real_backward_leaves_are_consumed_as_they_are(dev):
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    P = 400
    sc = make_scene(P, S=4, seed=4, log_scale_mean=-2.5)
    m = scene_model(sc, dev)
    m._scaling.requires_grad_(False)  # an untrained group: its .grad stays None
    cam = TorchCamera(make_camera(64, 64, yaw=0.3, pitch=-0.2), dev)
    out = render(cam, m, PipelineParams(), torch.tensor([0.1, 0.2, 0.3], device=dev))
    gen = torch.Generator().manual_seed(0)
    w = torch.randn(out["render"].shape, generator=gen).to(dev)
    (out["render"] * w).sum().backward()
    assert m._scaling.grad is None and m._xyz.grad is not None and m._features_rest.grad is not None
    arrays, grads = host(m)
    assert grads["_scaling"] is None and np.abs(grads["_features_rest"]).max() > 0 and np.abs(grads["_rotation"]).max() > 0
    sel = (torch.rand(P, generator=gen) < 0.5)
    res = pose.gradient(m, sel.to(dev), pivot="centroid")
    centroid = edit.selection_bounds(m._xyz.detach(), sel.to(dev))["centroid"].cpu().numpy()
    got, _, mags = assert_gate(res, arrays, grads, sel.numpy(), centroid, "backward")
    assert np.all(got[:6] != 0) and np.all(mags > 0)
    cam_grad = pose.camera_gradient(m, pivot=cam.camera_center)
    assert bool(cam_grad["rotation"].abs().sum() > 0)


# ---- 5. fit -----------------------------------------------------------------------------------------------------------------
def test_fit_brings_a_displaced_cluster_back(dev):
    """A compact cluster inside a scene, displaced by a tenth of its extent and a 3 degree turn; the targets are renders of the
    unedited model from three views.  Conditions only: the loss falls, the centroid ends nearer its place than it started, the
    returned composite reproduces the rows within the summed fp32 bounds of the edits, unselected rows keep their bits."""
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    P, n_cluster, iterations = 400, 80, 40
    sc = make_scene(P, S=4, seed=6, log_scale_mean=-2.5)
    rng = np.random.default_rng(6)
    sc.means3D[:n_cluster] = (np.array([0.3, 0.1, 0.0]) + 0.15 * rng.normal(size=(n_cluster, 3))).astype(np.float32)
    sc.opacities[:n_cluster] = np.float32(0.9)
    m = scene_model(sc, dev)
    sel = torch.zeros(P, dtype=torch.bool, device=dev)
    sel[:n_cluster] = True
    cams = [TorchCamera(make_camera(64, 64, yaw=yaw, pitch=pitch), dev) for yaw, pitch in ((-0.5, 0.1), (0.0, -0.2), (0.6, 0.2))]
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = PipelineParams()
    with torch.no_grad():
        targets = [render(c, m, pipe, bg)["render"].detach().clone() for c in cams]
    home = edit.selection_bounds(m._xyz.detach(), sel)
    home_c = home["centroid"].cpu().numpy().astype(np.float64)
    extent = float((home["hi"] - home["lo"]).max())
    delta = 0.1 * extent * np.array([0.6, -0.48, 0.64])
    norm_delta = float(np.linalg.norm(delta))
    edit.transform(m, sel, rotation=pose.twist_rotation(math.radians(3.0) * np.array([0.0, 0.6, 0.8])), translation=delta,
                   pivot="centroid")
    params = [getattr(m, attr) for _, attr in dref.PARAMS]

    def closure():
        for p in params:
            p.grad = None
        loss = sum(((render(c, m, pipe, bg)["render"] - t) ** 2).mean() for c, t in zip(cams, targets))
        loss.backward()
        return loss

    before = {attr: getattr(m, attr).detach().cpu().numpy().copy() for _, attr in dref.PARAMS}
    start_c = edit.selection_bounds(m._xyz.detach(), sel)["centroid"].cpu().numpy().astype(np.float64)
    assert abs(np.linalg.norm(start_c - home_c) - norm_delta) < 1e-5
    R, t, s, history = pose.fit(m, sel, closure, iterations=iterations, lr_rotation=0.005, lr_translation=norm_delta / 10)
    final = float(closure().detach())
    after = {attr: getattr(m, attr).detach().cpu().numpy().copy() for _, attr in dref.PARAMS}
    end_c = edit.selection_bounds(m._xyz.detach(), sel)["centroid"].cpu().numpy().astype(np.float64)
    print(f"loss {history['loss'][0]:.6e} -> {final:.6e}; centroid distance {norm_delta:.5f} -> {np.linalg.norm(end_c - home_c):.5f}")
    assert len(history["loss"]) == len(history["steps"]) == iterations
    assert final < history["loss"][0]
    assert np.linalg.norm(end_c - home_c) < norm_delta
    # rows outside the selection, and every tensor the similarity does not move, keep their bits
    keep = ~sel.cpu().numpy()
    for attr in before:
        rows = keep if attr in pose.GRADS and attr != "_scaling" else np.ones(P, bool)
        assert np.array_equal(before[attr][rows].view(np.uint32), after[attr][rows].view(np.uint32)), attr
    # the composite x' = s R x + t, applied in float64 to the snapshot, is the model; the allowed error is the fp32 bound of every
    # edit (edit_reference), carried through the later ones: a rotation spreads an earlier error by |R|, |q|, |D|
    assert s == 1.0 and R.dtype == np.float64 and t.dtype == np.float64
    eff = sel.cpu().numpy()
    state = {k: before[k].astype(np.float64) for k in ref.KEYS}
    bound = {k: np.zeros_like(state[k][eff]) for k in ("_xyz", "_rotation", "_features_rest")}
    for step in history["steps"]:
        c = eref.constants(**step, dtype=np.float64)
        absD = [np.abs(D) for D in c["D"]]
        bound["_xyz"] = c["s"] * eref.rotate3(np.abs(c["R"]), bound["_xyz"]) + eref.position_bound(c, state["_xyz"][eff])
        bound["_rotation"] = eref._abs_quat(np.abs(c["q"]), bound["_rotation"]) + eref.quat_bound(c, state["_rotation"][eff])
        bound["_features_rest"] = eref.rotate_rest(absD, bound["_features_rest"]) + eref.rest_bound(c, state["_features_rest"][eff])
        state = eref.transform(state, eff, c)
    whole = eref.transform({k: before[k].astype(np.float64) for k in ref.KEYS}, eff,
                           eref.constants(rotation=R, translation=t, scale=s, dtype=np.float64))
    for k, b in bound.items():
        err = np.abs(after[k][eff].astype(np.float64) - whole[k][eff])
        print(f"{k}: max error {err.max():.3e}, max bound {b.max():.3e}")
        assert (err <= b).all(), k
        assert np.abs(after[k][eff] - before[k][eff]).max() > 100 * b.max(), k  # (the rows did move, far beyond the bound)
