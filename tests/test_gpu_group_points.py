"""semantic.group_points (gui/main.py:1595-1665) on the GPU: on a synthetic scene with two positive blobs A and B, a
negative blob and scattered positive strays, with the RES mask taken from a render of A alone, the refinement returns
exactly A's Gaussians, equals a test-side restatement of the reference's loop (numpy DBSCAN, render_gui, the unfused
decode, compute_mask_ratio), leaves the model's semantic mask alone, and gives the same with the geometry cache on."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests.dbscan_reference import dbscan_reference

pytestmark = pytest.mark.gpu

S, N_CODES, W, H = 16, 4, 128, 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _scene(dev):
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import make_camera
    from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, svm_score_fn
    rng = np.random.default_rng(5)
    unit = 2.0 ** -10

    def blob(c, k):
        return np.asarray(c) + rng.normal(0.0, 0.12, size=(k, 3))

    a, b, neg = blob((-1.0, 0.0, 0.0), 1500), blob((1.0, 0.0, 0.0), 1500), blob((0.0, 1.0, 0.0), 1500)
    strays = rng.uniform((-2.5, -2.0, -1.0), (2.5, 2.0, 1.0), size=(4000, 3))
    far = np.min([np.linalg.norm(strays - np.asarray(c), axis=1) for c in ((-1, 0, 0), (1, 0, 0), (0, 1, 0))], axis=0) > 1.0
    strays = strays[far][:150]
    xyz = np.round(np.concatenate([a, b, neg, strays]) / unit) * unit
    P = len(xyz)
    kind = np.concatenate([np.zeros(1500), np.ones(1500), np.full(1500, 2), np.full(len(strays), 3)]).astype(np.int64)
    order = rng.permutation(P)
    xyz, kind = xyz[order], kind[order]
    sem = np.zeros((P, S), np.float32)
    sem[kind != 2, 0] = 1.0  # positive
    sem[kind == 2, 1] = 1.0  # negative
    t = lambda v: torch.tensor(np.asarray(v, np.float32), device=dev)  # noqa: E731
    shs = np.zeros((P, 16, 3), np.float32)
    shs[:, 0, :] = 0.5
    pc = GaussianSet(t(xyz), t(np.full((P, 3), 0.03)), t(np.tile([1.0, 0, 0, 0], (P, 1))), t(np.full((P, 1), 0.9)), t(shs),
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
    cam = TorchCamera(make_camera(W, H, yaw=0.0), dev)
    return pc, torch.from_numpy(kind).to(dev), mlp, lut, svm_score_fn(svm), cam


def compute_mask_ratio(refer_mask, mask):  # utils/image_utils.py:36-48
    if not refer_mask.any():
        return 0
    intersection = torch.logical_and(refer_mask, mask)
    return (torch.count_nonzero(intersection) / torch.count_nonzero(refer_mask)).item()


def reference_group_points(pc, selected, cam, bg, mlp, lut, score_fn, res_mask, eps=0.35, min_samples=600):
    """gui/main.py:1595-1665 restated on this package (numpy DBSCAN, the unfused decode)."""
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import compute_similarity_reference
    target_mask = selected.clone()
    relative_points = pc.get_xyz[target_mask].detach().cpu().numpy()
    clusters, _ = dbscan_reference(relative_points, eps, min_samples)
    set_cluster = set(clusters.tolist())
    clusters = torch.from_numpy(clusters).to(target_mask.device)
    selected_indices = torch.where(target_mask == 1)[0]
    target_mask[:] = 0
    for i in set_cluster:
        if i == -1:
            continue
        tem = torch.zeros_like(target_mask)
        tem[selected_indices[torch.where(clusters == i)[0]]] = 1
        tem = tem.bool()
        pc.set_semantic_masks(tem)
        with torch.no_grad():
            out = render_gui(cam, pc, bg)
            out_semantic = out["semantics"].permute(1, 2, 0).detach().reshape(-1, S)
            cos_sim, _ = compute_similarity_reference(out_semantic, mlp, lut, score_fn)
            if cos_sim.sum() == 0:
                continue
            semantic_mask = (cos_sim > 0).reshape(-1, H, W)
        if compute_mask_ratio(semantic_mask, res_mask.reshape(1, H, W)) > 0.7:
            target_mask = target_mask | tem
    pc.set_semantic_masks(None)
    return target_mask


def _res_mask_of(pc, members, cam, bg, mlp, lut, score_fn):
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import compute_similarity
    pc.set_semantic_masks(members)
    with torch.no_grad():
        sem = render_gui(cam, pc, bg)["semantics"]
    pc.set_semantic_masks(None)
    return (compute_similarity(sem, mlp, lut, score_fn) > 0).reshape(H, W)


@pytest.mark.parametrize("cache", [False, True])
def test_group_points_keeps_the_blob_in_the_mask(dev, cache):
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.semantic import group_points, select_gaussians
    pc, kind, mlp, lut, score_fn, cam = _scene(dev)
    bg = torch.zeros(3, device=dev)
    selected = select_gaussians(pc, mlp, lut, score_fn)
    assert torch.equal(selected, kind != 2)
    res = _res_mask_of(pc, kind == 0, cam, bg, mlp, lut, score_fn)
    assert 0 < int(res.sum()) < H * W
    if cache:
        rasterizer.set_geometry_cache(1 << 30)
    try:
        assert pc._semantics_masks is None
        got = group_points(pc, selected, cam, bg, mlp, lut, score_fn, res)
        assert pc._semantics_masks is None  # left as found
        mark = torch.ones(pc.get_xyz.shape[0], dtype=torch.bool, device=dev)
        pc.set_semantic_masks(mark)
        saved = pc._semantics_masks
        again = group_points(pc, selected, cam, bg, mlp, lut, score_fn, res)
        assert pc._semantics_masks is saved
        pc.set_semantic_masks(None)
    finally:
        if cache:
            rasterizer.set_geometry_cache(0)
    assert got.dtype == torch.bool and torch.equal(got, again)
    assert torch.equal(got, kind == 0)
    want = reference_group_points(pc, selected, cam, bg, mlp, lut, score_fn, res)
    assert torch.equal(got, want)
