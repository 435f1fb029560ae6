"""goi_hyperplane_amd.smooth on the GPU (csrc/smooth.hip), on the cases of tests/smooth_cases.py:

  1. transpose: in_ptr and in_edge integer-equal to the restatement, -1 tail included;
  2. loss: the gradient BIT-EQUAL to the float32 restatement (tests/smooth_reference.py), the scalar within gamma(n) L of the
     float64 one, N_E equal, exact zeros when N_E = 0, and both within the same derived bounds of torch autograd in float64 (CPU);
  3. the same bits on a second call and with the transpose passed or rebuilt; upstream 0.5 halves the bits exactly; no gradient
     is allocated without requires_grad; nothing synchronises;
  4. diffuse and complete_features bit-equal to the restatement for 1 and 5 iterations, the input untouched;
  5. one backward through render(...)["semantics"].sum() + smooth.loss(sem, ...) leaves the sum of the two gradients;
  6. ten gradient steps of size N_E / (4 d_max) on the device never increase the loss."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import knn, smooth
from tests import smooth_cases as sc
from tests import smooth_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def up(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)  # (a copy: the cases are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def on_device(name):
    """the case's tensors on the GPU and one forward with gradient: (f, idx, weight, rows, T, L, N_E, grad), computed once"""
    dev = torch.device("cuda:0")
    c = sc.case(name)
    f = up(c["f"], dev).requires_grad_(True)
    idx, w, rows = up(c["idx"], dev), up(c["weight"], dev), up(c["rows"], dev)
    T = smooth.transpose(idx)
    L, ne = smooth.loss_terms(f, idx, w, rows, T)
    L.backward()
    return f, idx, w, rows, T, L.detach().cpu().numpy(), int(ne.cpu()), f.grad.cpu().numpy().copy()


# ---- 1. the transpose --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.names())
def test_transpose_equals_the_restatement(dev, name):
    T = on_device(name)[4]
    in_ptr, in_edge = sc.transposed(name)
    assert T[0].dtype == T[1].dtype == torch.int32
    assert np.array_equal(T[0].cpu().numpy(), in_ptr)
    assert np.array_equal(T[1].cpu().numpy(), in_edge)
    assert np.all(T[1].cpu().numpy()[in_ptr[-1]:] == -1)


def test_transpose_of_an_empty_graph(dev):
    in_ptr, in_edge = smooth.transpose(torch.zeros((0, 4), dtype=torch.int32, device=dev))
    assert in_ptr.tolist() == [0] and in_edge.numel() == 0


# ---- 2. loss and gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.names())
def test_gradient_to_the_bit_and_loss_within_its_bound(dev, name):
    c = sc.case(name)
    S, k = c["f"].shape[1], c["idx"].shape[1]
    _, _, _, _, _, L, ne, grad = on_device(name)
    L32, g32, ne_ref = sc.reference(name, np.float32)
    L64, g64, _ = sc.reference(name, np.float64)
    bound = ref.gamma(ref.loss_chain(S, k)) * float(L64)
    print(f"{name}: L = {float(L)!r}, float64 {float(L64)!r}, |diff| = {abs(float(L) - float(L64)):.3e}, bound {bound:.3e}; "
          f"N_E = {ne}; gradient elements that differ from the float32 restatement: {int((bits(grad) != bits(g32)).sum())}")
    assert ne == ne_ref
    assert L.dtype == np.float32 and grad.dtype == np.float32
    assert np.array_equal(bits(grad), bits(g32))
    assert abs(float(L) - float(L64)) <= bound
    if ne == 0:
        assert bits(L) == 0 and not bits(grad).any()
    # torch autograd in float64 on the CPU, from the literal formula
    La, ga = sc.autograd64(name)
    assert abs(float(L) - La) <= ref.gamma(ref.loss_chain(S, k)) * La + 1e-12 * abs(La)
    assert np.all(np.abs(grad.astype(np.float64) - ga) <= sc.gradient_bound(name) + 1e-12 * np.abs(ga).max())


@pytest.mark.parametrize("name", ["knn_P1000_S16_k16", "star_weighted_P5000_S3_k1", "two_hubs_P1000_S17_k16", "knn_P65_S32_k3"])
def test_same_bits_again_with_the_transpose_rebuilt_and_under_half_the_upstream(dev, name):
    f, idx, w, rows, T, L, ne, grad = on_device(name)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # neither forward nor backward synchronises the host
    try:
        f2 = f.detach().clone().requires_grad_(True)
        L2, ne2 = smooth.loss_terms(f2, idx, w, rows, T)
        L2.backward()
        f3 = f.detach().clone().requires_grad_(True)
        L3 = smooth.loss(f3, idx, w, rows)  # the transpose is rebuilt
        (0.5 * L3).backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert bits(L2.detach().cpu().numpy()) == bits(L) and int(ne2.cpu()) == ne
    assert np.array_equal(bits(f2.grad.cpu().numpy()), bits(grad))
    assert bits(L3.detach().cpu().numpy()) == bits(L)
    assert np.array_equal(f3.grad.cpu().numpy(), np.float32(0.5) * grad)
    assert np.abs(grad).min() == 0 or np.abs(grad)[grad != 0].min() > 2 ** -120  # (halving is exact: nothing near the subnormals)


def test_no_gradient_is_allocated_without_requires_grad(dev):
    name = "knn_P1000_S32_k1"
    f, idx, w, rows, T, L, ne, _ = on_device(name)
    plain = f.detach()
    grad_bytes = plain.numel() * 4
    for run in (lambda: smooth.loss(plain, idx, w, rows, T), lambda: smooth.loss(plain, idx, w, rows)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = run()
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated(dev) - before < grad_bytes
        assert out.grad_fn is None and not out.requires_grad and out.dim() == 0 and out.dtype == torch.float32
        assert bits(out.cpu().numpy()) == bits(L)
    with torch.no_grad():
        out = smooth.loss(f, idx, w, rows, T)
    assert out.grad_fn is None and bits(out.cpu().numpy()) == bits(L)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = smooth.loss(f.detach().clone().requires_grad_(True), idx, w, rows, T)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated(dev) - before >= grad_bytes and out.grad_fn is not None


def test_empty_model(dev):
    f = torch.zeros((0, 8), device=dev, requires_grad=True)
    idx = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    L, ne = smooth.loss_terms(f, idx)
    L.backward()
    assert float(L.detach()) == 0 and int(ne) == 0 and f.grad.shape == (0, 8)
    assert smooth.diffuse(f.detach(), idx, iterations=3).shape == (0, 8)


def test_strided_features_are_made_contiguous(dev):
    name = "knn_P65_S32_k3"
    f, idx, w, rows, T, L, ne, grad = on_device(name)
    wide = torch.zeros((65, 40), device=dev)
    wide[:, :32] = f.detach()
    view = wide[:, :32].requires_grad_(True)
    smooth.loss(view, idx, w, rows, T).backward()
    assert np.array_equal(bits(view.grad.cpu().numpy()), bits(grad))


# ---- 4. diffusion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["knn_P63_S16_k8", "knn_P257_S3_k8", "tails_P257_S17_k8", "self_edges_P64_S32_k3", "random_P1000_S1_k16",
                                  "ids_out_of_range_P65_S16_k3", "knn_P1000_S16_k16", "star_weighted_P5000_S3_k1", "knn_P1_S1_k1"])
def test_diffuse_equals_the_restatement_bit_for_bit(dev, name):
    c = sc.case(name)
    f, idx, w = up(c["f"], dev), up(c["idx"], dev), up(c["weight"], dev)
    P = c["f"].shape[0]
    fixed = np.random.default_rng(3).random(P) < 0.3
    for lam, fx in ((1.0, fixed), (0.5, fixed), (0.3, None)):
        for iterations in (1, 5):
            got = smooth.diffuse(f, idx, w, up(fx, dev), lam, iterations)
            want = ref.diffuse(c["f"], c["idx"], c["weight"], fx, lam, iterations, np.float32)
            assert got.data_ptr() != f.data_ptr()
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (name, lam, iterations)
    assert np.array_equal(bits(f.cpu().numpy()), bits(c["f"]))  # the input is untouched
    assert torch.equal(smooth.diffuse(f, idx, w, None, 1.0, 0), f)


@pytest.mark.parametrize("name", ["knn_P257_S3_k8", "knn_P1000_S16_k16"])
def test_complete_features_is_graph_then_diffusion_with_the_known_rows_fixed(dev, name):
    c = sc.case(name)
    P = c["f"].shape[0]
    xyz, f = up(c["xyz"], dev), up(c["f"], dev)
    rng = np.random.default_rng(5)
    known = rng.random(P) < 0.25
    sel = rng.random(P) < 0.8
    for k, selection in ((8, None), (3, sel)):
        idx, _ = knn.graph(xyz, k, up(selection, dev))
        idx = idx.cpu().numpy()
        for iterations in (1, 5):
            got = smooth.complete_features(xyz, f, up(known, dev), k=k, iterations=iterations, selection=up(selection, dev))
            want = ref.diffuse(c["f"], idx, None, known, 1.0, iterations, np.float32)
            assert np.array_equal(bits(got.cpu().numpy()), bits(want))
            assert np.array_equal(bits(got.cpu().numpy()[known]), bits(c["f"][known]))
            if selection is not None:
                assert np.array_equal(bits(got.cpu().numpy()[~sel]), bits(c["f"][~sel]))
    assert np.array_equal(bits(f.cpu().numpy()), bits(c["f"]))
    # the graph of a cloud case IS what knn.graph returns for it
    assert np.array_equal(knn.graph(xyz, c["idx"].shape[1])[0].cpu().numpy(), c["idx"])


def test_gaussian_weights(dev):
    d2 = sc.case("knn_P63_S16_k8")["dist2"].copy()
    d2[::3, 5:] = np.inf  # the +inf of a row's -1 tail
    w = smooth.gaussian_weights(up(d2, dev), 0.7).cpu().numpy()
    arg = np.where(np.isfinite(d2), d2.astype(np.float64) / (2 * 0.7 ** 2), 0.0)
    want = np.where(np.isfinite(d2), np.exp(-arg), 0.0)
    assert w.dtype == np.float32 and w.shape == d2.shape and np.all(w[~np.isfinite(d2)] == 0) and np.all(w[np.isfinite(d2)] > 0)
    # torch glue in fp32: the argument is rounded twice (relative 2^-23 of |arg|, which is an absolute error of exp's exponent)
    assert np.all(np.abs(w - want) <= (arg + 4) * 2.0 ** -22 * want)


# ---- 5. with the rasterizer in one backward ---------------------------------------------------------------------------------------
def test_one_backward_through_render_and_the_regulariser_adds_the_two_gradients(dev):
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera, make_scene
    P = 400
    pc = GaussianSet.from_scene(make_scene(P, S=4, seed=4, log_scale_mean=-2.5), dev)
    cam = TorchCamera(make_camera(64, 64, yaw=0.3, pitch=-0.2), dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    sem = pc._semantics
    idx, dist2 = knn.graph(pc.get_xyz.detach(), 8)
    w = smooth.gaussian_weights(dist2, 0.5)
    T = smooth.transpose(idx)

    def grad_of(make):
        sem.grad = None
        make().backward()
        return sem.grad.detach().cpu().numpy().copy()

    g_render = grad_of(lambda: render(cam, pc, PipelineParams(), bg)["semantics"].sum())
    g_smooth = grad_of(lambda: smooth.loss(sem, idx, w, transposed=T))
    g_both = grad_of(lambda: render(cam, pc, PipelineParams(), bg)["semantics"].sum() + smooth.loss(sem, idx, w, transposed=T))
    assert np.abs(g_render).max() > 0 and np.abs(g_smooth).max() > 0
    # both addends are fp32 and autograd adds them once, in an order that is not ours: within 1 ulp of the larger addend
    ulp = np.spacing(np.maximum(np.abs(g_render), np.abs(g_smooth)))
    assert np.all(np.abs(g_both.astype(np.float64) - (g_render.astype(np.float64) + g_smooth.astype(np.float64))) <= ulp)


# ---- 6. descent on the device ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["knn_P257_S3_k8", "knn_P1000_S16_k16", "two_hubs_P1000_S17_k16"])
def test_ten_gradient_steps_on_the_device_never_increase_the_loss(dev, name):
    c = sc.case(name)
    S, k = c["f"].shape[1], c["idx"].shape[1]
    f0, idx, w, rows, T, _, ne, _ = on_device(name)
    d_max = ref.weight_degree(c["idx"], c["weight"], c["rows"])
    step = ne / (4 * d_max)
    f = f0.detach().clone().requires_grad_(True)
    losses = []
    for _ in range(11):
        f.grad = None
        L = smooth.loss(f, idx, w, rows, T)
        L.backward()
        losses.append(L.detach())
        with torch.no_grad():
            f -= step * f.grad
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print(name, losses)
    g = ref.gamma(ref.loss_chain(S, k))
    assert all(b <= a * (1 + g) for a, b in zip(losses, losses[1:]))
    assert losses[-1] < losses[0]
