"""The hyperplane fine-tune on the GPU (csrc/osh.hip: osh_counts_k, osh_fit_k) against the reference's own loop pinned in
tests/golden/ref_osh_pins.npz (gui/main.py:1673-1763 on CPU fp32), against the per-pixel LinearSVM.step loop on the same
GPU, and against itself (paths, batches, repeated runs)."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests.osh_reference import counts_of, fit_per_code, iou_flips

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ("a", "b", "c", "d")
# The IoU of an epoch is decided by the signs of the margins; after hundreds of steps a margin can oscillate within ~1e-5
# of 0, where fp32 summation order decides it.  The gates below therefore require the same epoch count and init IoU, and
# the same IoU trace up to isolated epochs (at most max(2, epochs / 200); the fixture's own float64 cross-check sees up to 19 in 8000 epochs).


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLD, "ref_osh_pins.npz"))


def _with_path(path, fn, *a, **k):
    from goi_hyperplane_amd import _lib
    _lib.set_option("osh_path", path)
    try:
        return fn(*a, **k)
    finally:
        _lib.set_option("osh_path", 0)


def _fit_case(pins, name, dev, path=0, K=1, max_epochs=8000, target_iou=0.9):
    from goi_hyperplane_amd.semantic import fit_hyperplanes_counts
    lut = torch.tensor(pins[f"{name}_lut"], device=dev)
    counts = torch.tensor(counts_of(pins[f"{name}_idx"], pins[f"{name}_gt"], lut.shape[0]), dtype=torch.int32, device=dev)
    w0 = torch.tensor(pins[f"{name}_w0"], device=dev).reshape(1, -1).repeat(K, 1)
    b0 = torch.tensor(pins[f"{name}_b0"], device=dev).reshape(1).repeat(K)
    HW = int(np.prod(pins[f"{name}_hw"]))
    return _with_path(path, fit_hyperplanes_counts, lut, counts.unsqueeze(0).repeat(K, 1, 1), HW, w0, b0,
                      max_epochs=max_epochs, target_iou=target_iou, return_trace=True)


def _assert_matches(fit, w, b, trace_ref, epochs_ref, init_ref, w_ref, b_ref, what):
    assert fit.epochs == epochs_ref, (what, fit.epochs, epochs_ref)
    np.testing.assert_array_equal(np.asarray(fit.init_iou), np.asarray(init_ref), err_msg=what)
    t = fit.trace.numpy()
    assert iou_flips(t[:, 1], trace_ref[:, 1]) <= max(2, epochs_ref // 200), what  # IoU trace: all but isolated epochs
    # loss: the first epoch (same w, no drift yet) to 1e-5; later epochs carry the drift of w between two fp32 fits (the
    # fixture's own loss trace differs from the exact float64 fit by up to 5e-4 relative over 8000 epochs)
    np.testing.assert_allclose(t[:1, 0], trace_ref[:1, 0], rtol=1e-5, atol=0, err_msg=what)
    np.testing.assert_allclose(t[:, 0], trace_ref[:, 0], rtol=1e-3, atol=1e-7, err_msg=what)
    scale = float(np.abs(w_ref).max())
    assert np.abs(w.cpu().numpy().reshape(-1) - w_ref.reshape(-1)).max() <= 1e-3 * scale, what
    assert abs(float(np.asarray(b.cpu() if torch.is_tensor(b) else b).reshape(-1)[0]) - float(np.asarray(b_ref).reshape(-1)[0])) \
        <= 1e-3 * scale, what


def test_osh_counts_equal_bincount(dev):
    from goi_hyperplane_amd.semantic import osh_counts
    g = torch.Generator(device=dev).manual_seed(3)
    for n_codes, HW in ((1, 4097), (37, 1056 * 1600), (300, 1056 * 1600), (1000, 512 * 512), (300, 1), (1000, 777)):
        idx = torch.randint(0, n_codes, (HW,), device=dev, generator=g, dtype=torch.int32)
        pos = torch.rand(HW, device=dev, generator=g) < 0.3
        got = osh_counts(idx, pos, n_codes)
        want = torch.stack([torch.bincount(idx[pos].long(), minlength=n_codes),
                            torch.bincount(idx[~pos].long(), minlength=n_codes)]).int()
        assert torch.equal(got, want), (n_codes, HW)
        assert torch.equal(osh_counts(idx, pos.to(torch.uint8), n_codes), want)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("path", (0, 1))
def test_fit_matches_reference_pins(dev, pins, name, path):
    """Both kernel paths on the fixture's counts: epochs and init IoU exactly the reference's, the IoU trace up to isolated
    epochs, the loss trace as in _assert_matches, final w / b within 1e-3 of max|w|."""
    w, b, fits = _fit_case(pins, name, dev, path)
    _assert_matches(fits[0], w, b[0], pins[f"{name}_trace"], int(pins[f"{name}_epochs"]), pins[f"{name}_init_iou"],
                    pins[f"{name}_w"], pins[f"{name}_b"], f"case {name} path {path}")
    if name == "c":  # empty mask: one epoch, NaN IoU
        assert fits[0].epochs == 1 and np.isnan(fits[0].iou)
    if name == "a":
        assert fits[0].epochs < 8000 and fits[0].iou >= 0.9
    if name == "b":
        assert fits[0].epochs == 8000


def test_fit_paths_batches_and_reruns_are_bit_identical(dev, pins):
    w1, b1, f1 = _fit_case(pins, "a", dev, 0)
    w2, b2, f2 = _fit_case(pins, "a", dev, 0)
    assert torch.equal(w1, w2) and torch.equal(b1, b2) and torch.equal(f1[0].trace, f2[0].trace)
    wg, bg, fg = _fit_case(pins, "a", dev, 1)  # the generic path: same arithmetic in the same order
    diff = (f1[0].trace != fg[0].trace).nonzero()
    assert torch.equal(w1, wg) and torch.equal(b1, bg) and diff.numel() == 0, \
        (diff[:6].tolist(), [(f1[0].trace[i, j].item(), fg[0].trace[i, j].item()) for i, j in diff[:6].tolist()])
    # a batch of three different fits equals three single fits bit for bit
    from goi_hyperplane_amd.semantic import fit_hyperplanes_counts
    lut = torch.tensor(pins["a_lut"], device=dev)
    idx, gt = pins["a_idx"], pins["a_gt"]
    masks = [gt, 1 - gt, (np.arange(gt.size) % 3 == 0).astype(np.uint8)]
    counts = torch.tensor(np.stack([counts_of(idx, m, 300) for m in masks]), dtype=torch.int32, device=dev)
    rng = np.random.default_rng(5)
    w0 = torch.tensor(rng.normal(size=(3, 256)).astype(np.float32) * 0.06, device=dev)
    b0 = torch.tensor([0.1, -0.2, 0.3], device=dev)
    wk, bk, fk = fit_hyperplanes_counts(lut, counts, 4096, w0, b0, max_epochs=3000, return_trace=True)
    for i in range(3):
        ws, bs, fs = fit_hyperplanes_counts(lut, counts[i:i + 1], 4096, w0[i:i + 1], b0[i:i + 1], max_epochs=3000,
                                            return_trace=True)
        assert torch.equal(ws[0], wk[i]) and torch.equal(bs[0], bk[i]), i
        assert fs[0].epochs == fk[i].epochs and torch.equal(fs[0].trace, fk[i].trace), i


def test_fit_all_positive_and_degenerate_inputs(dev, pins):
    from goi_hyperplane_amd.semantic import fit_hyperplanes_counts
    lut_np = pins["d_lut"]
    idx = pins["d_idx"]
    counts_np = counts_of(idx, np.ones_like(idx), lut_np.shape[0])
    w0 = pins["d_w0"]
    ref = fit_per_code(lut_np, counts_np, idx.size, w0, float(pins["d_b0"]), max_epochs=500)
    lut = torch.tensor(lut_np, device=dev)
    counts = torch.tensor(counts_np, dtype=torch.int32, device=dev).unsqueeze(0)
    for path in (0, 1):
        w, b, fits = _with_path(path, fit_hyperplanes_counts, lut, counts, idx.size, torch.tensor(w0, device=dev)[None],
                                torch.tensor(pins["d_b0"], device=dev).reshape(1), max_epochs=500, return_trace=True)
        assert fits[0].epochs == ref["epochs"]
        assert iou_flips(fits[0].trace.numpy()[:, 1], ref["trace"][:, 1]) == 0
    # a present code with an all-zero LUT row
    lut0 = lut.clone()
    lut0[int(idx[0])] = 0
    with pytest.raises(ValueError):
        fit_hyperplanes_counts(lut0, counts, idx.size, torch.tensor(w0, device=dev)[None],
                               torch.tensor(pins["d_b0"], device=dev).reshape(1))
    # ABI limits
    with pytest.raises(ValueError):
        fit_hyperplanes_counts(lut, counts, idx.size, torch.tensor(w0, device=dev)[None],
                               torch.tensor(pins["d_b0"], device=dev).reshape(1), max_epochs=1_000_001)


def _scene_frame(dev, n_codes=300, S=16, W=512, H=512):
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera, make_scene
    from goi_hyperplane_amd.semantic import SemanticModel
    sc = make_scene(20000, S=S, seed=4, log_scale_mean=-3.0)
    pc = GaussianSet.from_scene(sc, dev)
    with torch.no_grad():
        out = render(TorchCamera(make_camera(W, H, yaw=0.2), dev), pc, PipelineParams(), torch.zeros(3, device=dev))
    torch.manual_seed(8)
    mlp = SemanticModel(dim_in=S, dim_out=n_codes, num_layer=1, use_bias=True, device=dev)
    pos_code = torch.rand(n_codes, device=dev) < 0.3
    u = torch.nn.functional.normalize(torch.randn(256, device=dev), dim=0)
    lut = torch.randn(n_codes, 256, device=dev) * 0.1 + 0.2 * (2 * pos_code.float() - 1)[:, None] * u[None]
    return pc, out["semantics"].detach(), mlp, lut, pos_code, u


def test_fit_hyperplane_end_to_end_matches_per_pixel_loop(dev):
    """512x512 rendered frame: fit_hyperplane against the reference's per-pixel LinearSVM.step loop on the same GPU and
    the same decoded codes (capped at 2000 epochs)."""
    from goi_hyperplane_amd.semantic import LinearSVM, _decode_idx, fit_hyperplane
    pc, sem, mlp, lut, pos_code, u = _scene_frame(dev)
    idx = _decode_idx(sem, mlp, lut.shape[0]).long()
    positive = pos_code[idx]                                   # the "RES mask": the pixels of the positive codes
    text = torch.nn.functional.normalize(0.3 * u + 0.7 * torch.nn.functional.normalize(torch.randn(256, device=dev), dim=0),
                                         dim=0)
    svm_ref = LinearSVM(set_bias=0.86).to(dev)
    svm_ref.weight_set(text.reshape(1, -1))
    svm = LinearSVM(set_bias=0.86).to(dev)
    svm.weight_set(text.reshape(1, -1))
    fit = fit_hyperplane(sem, mlp, lut, positive, svm, max_epochs=2000, return_trace=True)

    feat = lut[idx]
    normed = feat / feat.norm(dim=-1, keepdim=True)
    gt = positive.float().reshape(-1, 1)
    init_iou = svm_ref.eval_forward(normed, gt)
    trace, iou, epoch = [], 0, 0
    while epoch < 2000 and iou < 0.9:
        loss, iou = svm_ref.step(normed, gt)
        trace.append((loss.item(), iou))
        epoch += 1
    trace = np.array(trace)
    _assert_matches(fit, svm.linear.weight.detach(), svm.linear.bias.detach(), trace, epoch, init_iou,
                    svm_ref.linear.weight.detach().cpu().numpy(), svm_ref.linear.bias.detach().cpu().numpy(), "end to end")
    assert fit.loss == pytest.approx(trace[-1, 0], rel=1e-3)


def test_fit_hyperplane_input_errors(dev):
    from goi_hyperplane_amd.semantic import LinearSVM, fit_hyperplane
    pc, sem, mlp, lut, pos_code, u = _scene_frame(dev, W=64, H=48)
    svm = LinearSVM().to(dev)
    bad = torch.zeros(48 * 64, device=dev)
    bad[5] = 2.0
    w_before = svm.linear.weight.detach().clone()
    with pytest.raises(ValueError):
        fit_hyperplane(sem, mlp, lut, bad, svm)
    assert torch.equal(svm.linear.weight.detach(), w_before)  # nothing written on a rejected mask
    with pytest.raises(ValueError):
        fit_hyperplane(sem, mlp, lut, torch.zeros(48 * 64 + 1, device=dev), svm)
    # an empty mask: the IoU is 0 while any pixel is predicted and NaN once none is; from a hyperplane that predicts
    # nothing the fit stops after its first epoch
    fit = fit_hyperplane(sem, mlp, lut, torch.zeros(48, 64, dtype=torch.bool, device=dev), svm)
    assert np.isnan(fit.iou)
    with torch.no_grad():
        svm.linear.bias.fill_(-10.0)
    fit = fit_hyperplane(sem, mlp, lut, torch.zeros(48, 64, dtype=torch.bool, device=dev), svm)
    assert fit.epochs == 1 and np.isnan(fit.iou) and np.isnan(fit.init_iou)


def test_select_gaussians_matches_reference_decode(dev):
    from goi_hyperplane_amd.semantic import LinearSVM, compute_similarity_reference, select_gaussians, svm_score_fn
    pc, sem, mlp, lut, pos_code, u = _scene_frame(dev, W=64, H=48)
    svm = LinearSVM().to(dev)
    svm.weight_set(u.reshape(1, -1))
    mask = select_gaussians(pc, mlp, lut, svm_score_fn(svm))
    feats = pc.get_semantics.detach()
    sim_r, idx_r = compute_similarity_reference(feats, mlp, lut, svm_score_fn(svm), 0.5)
    from goi_hyperplane_amd.semantic import _decode_idx
    idx_f = _decode_idx(feats.t().contiguous(), mlp, lut.shape[0]).long()
    agree = idx_f == idx_r                   # the argmax may differ from the GEMM-based reference only on near ties
    assert mask.dtype == torch.bool and mask.shape == (feats.shape[0],)
    assert agree.float().mean().item() > 0.9999
    assert torch.equal(mask[agree], (sim_r > 0)[agree])
    assert 0 < int(mask.sum()) < feats.shape[0]
