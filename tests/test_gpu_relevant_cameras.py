"""semantic.relevant_cameras (gui/main.py:407-478) and semantic.evaluate_cameras (gui/main.py:1957-2016) on the GPU.

The scene: one positive-code object blob and negative-code distractor blobs, seen by 12 cameras: some see the object
whole, some only a sliver at the frame's edge (count below 10 % of the largest), some do not see it at all.  The sweep
equals a test-side restatement of the reference's precompute (render_gui, the fused decode, torch.count_nonzero, a host
dilation by scipy.ndimage.binary_dilation standing in for cv2.dilate, >= 0.5, and the reference's removal loop): kept
indices, counts, masks and dilated masks are equal.  The model's semantic mask is left as found, and the result is the
same with the geometry cache on.  evaluate_cameras equals a restatement of eval_epoch's loop with the formulas of
utils/image_utils.py:59-102 (pinned in tests/test_masks_cpu.py)."""
from __future__ import annotations

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

S, N_CODES, W, H = 16, 4, 160, 120
HALF_W = 5.0 * np.tan(0.5)  # the frame's half-width at distance 5 for fovx = 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _scene(dev):
    from goi_hyperplane_amd.render import GaussianSet
    from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, svm_score_fn
    rng = np.random.default_rng(11)

    def blob(c, k, s):
        return np.asarray(c) + rng.normal(0.0, s, size=(k, 3))

    obj = blob((0.0, 0.0, 0.0), 3000, 0.25)
    distractors = [blob((1.6, 0.9, 0.6), 1500, 0.2), blob((-1.6, -0.7, -0.5), 1500, 0.2), blob((0.0, 0.0, 6.0), 1500, 0.3)]
    xyz = np.concatenate([obj] + distractors)
    P = len(xyz)
    positive = np.zeros(P, bool)
    positive[: len(obj)] = True
    order = rng.permutation(P)
    xyz, positive = xyz[order], positive[order]
    sem = np.zeros((P, S), np.float32)
    sem[positive, 0] = 1.0
    sem[~positive, 1] = 1.0
    t = lambda v: torch.tensor(np.asarray(v, np.float32), device=dev)  # noqa: E731
    shs = np.zeros((P, 16, 3), np.float32)
    shs[:, 0, :] = 0.5
    pc = GaussianSet(t(xyz), t(np.full((P, 3), 0.04)), t(np.tile([1.0, 0, 0, 0], (P, 1))), t(np.full((P, 1), 0.9)), t(shs),
                     t(sem))
    torch.manual_seed(3)
    mlp = SemanticModel(dim_in=S, dim_out=N_CODES, num_layer=1, use_bias=True, device=dev)
    with torch.no_grad():
        lin = mlp.layers[0]
        lin.weight.zero_()
        lin.weight[0, 0] = 10.0
        lin.weight[1, 1] = 10.0
        lin.bias.copy_(torch.tensor([-1.0, 0.0, -5.0, -5.0]))
    u = torch.nn.functional.normalize(torch.randn(256, device=dev), dim=0)
    lut = torch.stack([u, -u, -u, -u]) + 0.01 * torch.randn(N_CODES, 256, device=dev)
    svm = LinearSVM().to(dev)
    svm.weight_set(u.reshape(1, -1))
    return pc, mlp, lut, svm_score_fn(svm)


def _cameras(dev):
    from goi_hyperplane_amd.render import TorchCamera
    from goi_hyperplane_amd.scene import make_camera
    specs = [dict(yaw=y, distance=3.5) for y in (0.0, 0.8, 1.6, 2.4, 3.2)]  # the whole object
    specs.insert(2, dict(yaw=0.0, distance=5.0, target=(HALF_W + 0.30, 0.0, 0.0)))  # slivers at the right edge
    specs.insert(4, dict(yaw=0.0, distance=5.0, target=(HALF_W + 0.45, 0.0, 0.0)))
    specs.append(dict(yaw=0.0, distance=5.0, target=(HALF_W + 0.60, 0.0, 0.0)))
    specs.insert(1, dict(yaw=0.0, distance=1.5, target=(0.0, 0.0, 4.0)))  # the object behind the camera
    specs.insert(7, dict(yaw=np.pi, distance=1.5, target=(0.0, 0.0, -4.0)))
    specs.append(dict(yaw=0.0, distance=1.5, target=(4.0, 0.0, 4.0)))
    specs.append(dict(yaw=0.4, distance=9.0))  # small but whole
    return [TorchCamera(make_camera(W, H, **s), dev) for s in specs]


def reference_precompute(cams, pc, mlp, lut, score_fn, thresh, bg):
    """gui/main.py:407-478 restated on this package: cv2.dilate(m, ones((3,3)), iterations=5) is scipy's binary dilation
    with the same square and border (tests/test_masks_cpu.py)."""
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import compute_similarity
    pc.set_semantic_masks()
    max_relative_number = 0
    min_relative_ratio = 0.1
    relative_cameras = []
    counts = []
    for ind, camera in enumerate(cams):
        out = render_gui(camera, pc, bg)
        cos_sim = compute_similarity(out["semantics"], mlp, lut, score_fn, thresh)
        counts.append(int(torch.count_nonzero(cos_sim)))
        if cos_sim.any():
            relative_pixel_number = torch.count_nonzero(cos_sim)
            max_relative_number = max(max_relative_number, relative_pixel_number)
            semantic_mask = (cos_sim > 0).reshape(H, W, -1).permute(2, 0, 1)
            dilated = semantic_mask.detach().to(dtype=torch.float32).cpu().numpy().squeeze(0)
            dilated = ndimage.binary_dilation(dilated, np.ones((3, 3), bool), iterations=5, border_value=0).astype(np.float32)
            dilated = dilated >= 0.5
            relative_cameras.append((ind, relative_pixel_number, semantic_mask,
                                     torch.from_numpy(dilated).unsqueeze(0).to(semantic_mask.device)))
    i = 0
    while i < len(relative_cameras):
        if relative_cameras[i][1] < max_relative_number * min_relative_ratio:
            relative_cameras.remove(relative_cameras[i])
        else:
            i += 1
    pc.set_semantic_masks(None)
    return relative_cameras, counts


@pytest.mark.parametrize("cache", [False, True])
def test_relevant_cameras_equal_the_reference_precompute(dev, cache):
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.semantic import relevant_cameras
    pc, mlp, lut, score_fn = _scene(dev)
    cams = _cameras(dev)
    bg = torch.zeros(3, device=dev)
    want, want_counts = reference_precompute(cams, pc, mlp, lut, score_fn, 0.5, bg)
    # the scene holds every case of the filter
    mx = max(want_counts)
    assert sum(c == 0 for c in want_counts) >= 3, want_counts
    assert any(0 < c < 0.1 * mx for c in want_counts), want_counts
    assert len(want) >= 5, want_counts
    mark = torch.zeros(pc.get_xyz.shape[0], dtype=torch.bool, device=dev)
    mark[::3] = True
    pc.set_semantic_masks(mark)  # the sweep clears it, as the reference does, and puts it back
    saved = pc._semantics_masks
    if cache:
        rasterizer.set_geometry_cache(1 << 30)
    try:
        got = relevant_cameras(cams, pc, mlp, lut, score_fn, 0.5, bg)
        again = relevant_cameras(cams, pc, mlp, lut, score_fn, 0.5, bg)
    finally:
        if cache:
            rasterizer.set_geometry_cache(0)
    assert pc._semantics_masks is saved
    pc.set_semantic_masks(None)
    assert got.index == [ind for ind, *_ in want]
    assert got.counts.dtype == torch.int64 and got.counts.tolist() == want_counts
    K = len(want)
    assert got.semantic_mask.shape == (K, 1, H, W) and got.semantic_mask.dtype == torch.bool
    assert got.semantic_mask_dilated.shape == (K, 1, H, W) and got.semantic_mask_dilated.dtype == torch.bool
    for k, (_, _, m, md) in enumerate(want):
        assert torch.equal(got.semantic_mask[k], m), k
        assert torch.equal(got.semantic_mask_dilated[k], md), k
    assert again.index == got.index and torch.equal(again.semantic_mask_dilated, got.semantic_mask_dilated)


def test_relevant_cameras_refuse_mixed_frames(dev):
    from goi_hyperplane_amd.render import TorchCamera
    from goi_hyperplane_amd.scene import make_camera
    from goi_hyperplane_amd.semantic import relevant_cameras
    pc, mlp, lut, score_fn = _scene(dev)
    cams = _cameras(dev)[:2] + [TorchCamera(make_camera(W, H + 2), dev)]
    with pytest.raises(ValueError, match="one frame size"):
        relevant_cameras(cams, pc, mlp, lut, score_fn, 0.5, torch.zeros(3, device=dev))


def _iou(label, pred):  # utils/image_utils.py:59-71
    pred_inds, label_inds = pred == 1, label == 1
    intersection = torch.logical_and(pred_inds, label_inds).sum()
    union = torch.logical_or(pred_inds, label_inds).sum()
    return float("nan") if union == 0 else float(intersection) / float(max(union, 1))


def _mpa(true_labels, predicted_labels):  # :74-88
    a1 = torch.sum((predicted_labels == 1) & (true_labels == 1)).float() / torch.sum(true_labels == 1).float()
    a0 = torch.sum((predicted_labels == 0) & (true_labels == 0)).float() / torch.sum(true_labels == 0).float()
    a1 = a1 if torch.sum(true_labels == 1) > 0 else torch.tensor(0.)
    a0 = a0 if torch.sum(true_labels == 0) > 0 else torch.tensor(0.)
    return (a1 + a0) / 2


def _mp(true_labels, predicted_labels):  # :92-102
    p1 = torch.sum((predicted_labels == 1) & (true_labels == 1)).float() / torch.sum(predicted_labels == 1).float()
    p0 = torch.sum((predicted_labels == 0) & (true_labels == 0)).float() / torch.sum(predicted_labels == 0).float()
    return (p1 + p0) / 2


def reference_eval(cams, gt_masks, pc, mlp, lut, score_fn, thresh, bg):
    """eval_epoch's loop (gui/main.py:1957-2016) on same-shape [H, W] masks, the metrics on the host."""
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import compute_similarity
    total_iou, total_mpa, total_mp = 0.0, 0.0, 0.0
    per = []
    for i, camera in enumerate(cams):
        out = render_gui(camera, pc, bg)
        pred_mask = (compute_similarity(out["semantics"], mlp, lut, score_fn, thresh) > 0).reshape(H, W).cpu()
        gt = gt_masks[i].cpu() != 0
        iou, mpa, mp = _iou(gt, pred_mask), _mpa(gt, pred_mask), _mp(gt, pred_mask)
        per.append((iou, mpa, mp))
        total_iou += iou
        total_mpa += mpa
        total_mp += mp
    n = len(cams)
    return per, total_iou / n, total_mpa / n, total_mp / n


def same(a, b):
    a, b = np.float64(a), np.float64(b)
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("gt_kind", ["shifted", "with_empty_view"])
def test_evaluate_cameras_equals_eval_epoch(dev, gt_kind):
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import compute_similarity, evaluate_cameras
    pc, mlp, lut, score_fn = _scene(dev)
    cams = _cameras(dev)
    bg = torch.ones(3, device=dev)
    V = len(cams)
    gt = torch.zeros((V, H, W), dtype=torch.uint8, device=dev)
    for v, cam in enumerate(cams):
        pred = (compute_similarity(render_gui(cam, pc, bg)["semantics"], mlp, lut, score_fn, 0.5) > 0).reshape(H, W)
        gt[v] = torch.roll(pred, shifts=(v % 3, 2 - v % 4), dims=(0, 1)).to(torch.uint8) * 255
        if not pred.any() and gt_kind == "shifted":
            gt[v, 10:20, 30:45] = 1  # a ground truth the prediction misses: IoU 0
    got = evaluate_cameras(cams, gt.float() if gt_kind == "shifted" else gt, pc, mlp, lut, score_fn, 0.5, bg)
    per, mean_iou, mean_mpa, mean_mp = reference_eval(cams, gt, pc, mlp, lut, score_fn, 0.5, bg)
    assert got.iou.dtype == torch.float64 and got.mpa.dtype == torch.float32 and got.mp.dtype == torch.float32
    for v, (iou, mpa, mp) in enumerate(per):
        assert same(got.iou[v], iou) and got.mpa[v].numpy().tobytes() == mpa.numpy().tobytes(), v
        assert got.mp[v].numpy().tobytes() == mp.numpy().tobytes() or (torch.isnan(got.mp[v]) and torch.isnan(mp)), v
    assert same(got.mean_iou, mean_iou) and same(got.mean_mpa, float(mean_mpa)) and same(got.mean_mp, float(mean_mp))
    if gt_kind == "with_empty_view":
        assert np.isnan(got.mean_iou)  # a view with neither prediction nor ground truth has no IoU, and the mean follows
    else:
        assert not np.isnan(got.mean_iou) and 0.0 < got.mean_iou < 1.0
