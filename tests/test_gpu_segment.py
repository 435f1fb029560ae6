"""goi_hyperplane_amd.segment on the GPU (csrc/segment.hip), on the cases of tests/segment_cases.py:

  1. join, root, size, label and count INTEGER-EQUAL to the restatement (tests/segment_reference.py) on every case, the status
     word 0, the inputs untouched, the same bits on a second call;
  2. the same bits under a permutation of the rows: join row for row, the partition as sets with ids mapped back;
  3. instances == knn.graph + edges + components made by hand, without a host synchronisation;
  4. select with several seeds, a -1 seed and a seed in a dropped component;
  5. end to end: two balls of Gaussians that touch (one cluster of positions) come apart by their features, and a click on one
     ball returns exactly that ball."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import knn, segment
from tests import segment_cases as sc
from tests import segment_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def up(a, dev=None):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev or torch.device("cuda:0"))  # (a copy: the cases are read-only)


def down(seg):
    return tuple(t.cpu().numpy() for t in (seg.root, seg.size, seg.label)) + (int(seg.count.cpu()[0]), int(seg.status.cpu()[0]))


def run(c, tensors=None):
    """the case through the module: (the device tensors, join or None, Segments)"""
    t = tensors or {key: up(c[key]) for key in ("idx", "f", "dist2", "labels", "rows", "join")}
    join = None
    if c["gate"]:
        join = segment.edges(t["idx"], t["f"], c["tau"], t["dist2"], c["max_dist2"], t["labels"], t["rows"], c["mutual"])
    used = t["join"] if c["join"] is not None else join
    return t, join, segment.components(t["idx"], used, t["rows"], c["min_size"])


@functools.lru_cache(maxsize=None)
def on_device(name):
    return run(sc.case(name))


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.names())
def test_every_output_equals_the_restatement(dev, name):
    c = sc.case(name)
    t, join, seg = on_device(name)
    want_join, want_root, want_size, want_label, want_count = sc.reference(name)
    root, size, label, count, status = down(seg)
    P, k = c["idx"].shape
    print(f"{name}: P = {P}, k = {k}, joins = {None if join is None else int(join.sum())}, count = {count} (reference {want_count}), "
          f"largest component = {int(size.max()) if P else 0}, status = {status}")
    assert status == 0
    if c["gate"]:
        assert join.dtype == torch.uint8 and tuple(join.shape) == (P, k)
        assert np.array_equal(join.cpu().numpy(), want_join)
    for got, want in ((root, want_root), (size, want_size), (label, want_label)):
        assert got.dtype == np.int32 and got.shape == (P,)
        assert np.array_equal(got, want)
    assert count == want_count
    assert seg.count.dtype == seg.status.dtype == torch.int32 and tuple(seg.count.shape) == (1,) and seg.graph is None
    # the inputs are untouched
    for key in ("idx", "f", "dist2", "labels", "rows", "join"):
        if c[key] is not None:
            assert np.array_equal(t[key].cpu().numpy().view(np.uint8), np.ascontiguousarray(c[key]).view(np.uint8)), key
    # the same bits on a second call, on the same tensors
    _, join2, seg2 = run(c, t)
    if c["gate"]:
        assert torch.equal(join, join2)
    again = down(seg2)
    assert all(np.array_equal(a, b) for a, b in zip(again, (root, size, label, count, status)))


# ---- 2. under a permutation of the rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sc.names() if sc.case(n)["idx"].shape[0] > 1])
def test_the_same_bits_under_a_permutation_of_the_rows(dev, name):
    c = sc.case(name)
    idx = c["idx"]
    P, k = idx.shape
    perm = np.random.default_rng(P + k).permutation(P)  # new row n is old row perm[n]
    inv = np.empty(P, np.int64)
    inv[perm] = np.arange(P)
    moved = idx[perm]
    inside = (moved >= 0) & (moved < P)
    moved = np.where(inside, inv[np.where(inside, moved, 0)], moved).astype(np.int32)  # -1 and ids out of range stay what they are
    pc = dict(c, idx=moved, **{key: None if c[key] is None else c[key][perm] for key in ("f", "dist2", "labels", "rows", "join")})
    _, join, seg = on_device(name)
    _, pjoin, pseg = run(pc)
    root, size, label, count, status = down(seg)
    proot, psize, plabel, pcount, pstatus = down(pseg)
    assert pstatus == 0 and pcount == count
    if c["gate"]:
        assert np.array_equal(pjoin.cpu().numpy(), join.cpu().numpy()[perm])
    assert {frozenset(perm[list(g)].tolist()) for g in ref.partition(proot)} == ref.partition(root)
    assert np.array_equal(psize, size[perm]) and np.array_equal(proot >= 0, (root >= 0)[perm])
    assert np.array_equal(plabel >= 0, (label >= 0)[perm])  # the same components are kept (their ranks follow the new roots)
    for g in ref.partition(root):  # the root is the smallest NEW id of the component
        new = inv[list(g)]
        assert np.all(proot[new] == new.min())


# ---- 3. instances --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,kw", [
    ("knn_P257_k8_S4", 8, dict(tau=0.12, min_size=3)),
    ("knn_P5000_k8_S16", 3, dict(tau=0.5, mutual=True, max_dist2=0.05, min_size=2, selection=True, labels=True)),
    ("knn_P63_k8_S16", 16, dict()),
])
def test_instances_is_graph_then_edges_then_components(dev, name, k, kw):
    c = sc.case(name)
    P = c["idx"].shape[0]
    rng = np.random.default_rng(11)
    kw = dict(kw)
    selection = up(rng.random(P) < 0.8) if kw.pop("selection", False) else None
    labels = up(rng.integers(-1, 3, P).astype(np.int64)) if kw.pop("labels", False) else None
    xyz, f = up(c["xyz"]), up(c["f"])
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # nothing here synchronises the host
    try:
        seg = segment.instances(xyz, f, k=k, labels=labels, selection=selection, **kw)
        idx, dist2 = knn.graph(xyz, k, selection)
        join = segment.edges(idx, f, kw.get("tau", float("inf")), dist2, kw.get("max_dist2"), labels, selection, kw.get("mutual", False))
        hand = segment.components(idx, join, selection, kw.get("min_size", 1))
        picked = segment.select(seg, torch.zeros(1, dtype=torch.int64, device=dev))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(seg.graph[0], idx) and torch.equal(seg.graph[1].view(torch.int32), dist2.view(torch.int32))
    assert torch.equal(seg.graph[2], join)
    for a, b in zip(seg[:5], hand[:5]):
        assert torch.equal(a, b)
    assert int(seg.status.cpu()[0]) == 0 and picked.dtype == torch.bool
    # and the three calls are what the restatement gives for the same graph
    want_join = ref.edges(idx.cpu().numpy(), c["f"], kw.get("tau", np.inf), dist2.cpu().numpy(), kw.get("max_dist2"),
                          None if labels is None else labels.cpu().numpy(), None if selection is None else selection.cpu().numpy(),
                          kw.get("mutual", False))
    assert np.array_equal(join.cpu().numpy(), want_join)
    want = ref.components(idx.cpu().numpy(), want_join, None if selection is None else selection.cpu().numpy(), kw.get("min_size", 1))
    got = down(seg)
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want))
    assert want_join.any() and (want_join.mean() < 1) == ("tau" in kw)  # the gate decides something; the defaults join every edge
    if selection is not None:
        assert np.all(got[0][~selection.cpu().numpy()] == -1)


def test_an_empty_model(dev):
    idx = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    join = segment.edges(idx, torch.zeros((0, 4), device=dev), 1.0)
    seg = segment.components(idx, join)
    assert tuple(join.shape) == (0, 3) and seg.label.numel() == seg.root.numel() == seg.size.numel() == 0
    assert seg.count.cpu().tolist() == [0] and seg.status.cpu().tolist() == [0]
    assert segment.select(seg, torch.tensor([0, -1], device=dev)).shape == (0,)


# ---- 4. select -----------------------------------------------------------------------------------------------------------------------
def test_select_with_several_seeds_a_missing_seed_and_a_dropped_component(dev):
    _, _, seg = on_device("sizes_min3")  # components {3}, {0, 9} dropped; {1, 4, 6} and {2, 5, 7, 8, 10} kept
    sel = lambda seeds, dtype=torch.int64: np.flatnonzero(segment.select(seg, torch.tensor(seeds, dtype=dtype, device=dev)).cpu().numpy()).tolist()  # noqa: E731
    assert sel([4]) == [1, 4, 6]
    assert sel([4, 10]) == [1, 2, 4, 5, 6, 7, 8, 10] == sel([[6, 1], [8, 8]])
    assert sel([-1]) == [] and sel([3]) == [] and sel([9, 0]) == [] and sel([]) == [] and sel([11, 2 ** 40, -5]) == []
    assert sel([-1, 3, 6, 0], torch.int32) == [1, 4, 6]
    out = segment.select(seg, torch.tensor([4], device=dev))
    assert out.dtype == torch.bool and tuple(out.shape) == (11,) and out.is_cuda
    _, _, none = on_device("sizes_min6")
    assert sel([4]) and not segment.select(none, torch.arange(11, device=dev)).any()
    _, _, big = on_device("knn_P5000_k8_S16")
    label = big.label.cpu().numpy()
    seeds = [int(np.flatnonzero(label == 0)[0]), int(np.flatnonzero(label == label.max())[-1]), -1, int(np.flatnonzero(label == -1)[0])]
    got = segment.select(big, torch.tensor(seeds, device=dev)).cpu().numpy()
    assert np.array_equal(got, (label == 0) | (label == label.max()))


# ---- 5. end to end: two balls that touch, and a click ----------------------------------------------------------------------------------
def test_two_touching_balls_come_apart_by_their_features_and_a_click_selects_one(dev):
    from goi_hyperplane_amd import cluster
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import make_camera, make_scene
    P, S = 2000, 16
    rng = np.random.default_rng(5)
    scene = make_scene(P, S=S, sh_degree=1, seed=3, log_scale_mean=-3.0)
    u = rng.standard_normal((P, 3))
    inside = u / np.linalg.norm(u, axis=1, keepdims=True) * (0.5 * rng.random((P, 1)) ** (1 / 3))  # uniform in a ball of radius 0.5
    ball = (np.arange(P) >= P // 2).astype(np.int64)  # ball A: rows 0 .. 999 around (-0.5, 0, 0); ball B around (+0.5, 0, 0)
    scene.means3D = (inside + np.stack([ball - 0.5, 0 * ball, 0 * ball], 1)).astype(np.float32)
    scene.semantics = (np.eye(S)[ball] + 0.01 * rng.standard_normal((P, S))).astype(np.float32)  # e0 or e1, plus noise
    pc = GaussianSet.from_scene(scene, dev)
    cam = make_camera(96, 64)
    tcam, bg = TorchCamera(cam, dev), torch.zeros(3, device=dev)
    xyz, sem = pc.get_xyz.detach(), pc._semantics.detach()

    # positions alone: ONE object (every edge joins), and one DBSCAN cluster at the graph's own scale
    whole = segment.instances(xyz, None, k=8)
    assert whole.count.cpu().tolist() == [1] and whole.size.cpu().unique().tolist() == [P]
    eps = float(whole.graph[1][:, -1].max().sqrt())
    assert len(set(cluster.dbscan(xyz, eps, 4).cpu().tolist()) - {-1}) == 1
    # with the features: exactly the two constructed sets
    seg = segment.instances(xyz, sem, k=8, tau=0.5)
    label = seg.label.cpu().numpy()
    assert seg.status.cpu().tolist() == [0] and seg.count.cpu().tolist() == [2]
    assert np.array_equal(label, ball) and seg.root.cpu().unique().tolist() == [0, P // 2]
    assert seg.size.cpu().unique().tolist() == [P // 2]
    # the click: a pixel over ball A
    centre = np.array([-0.5, 0.0, 0.0, 1.0], np.float32) @ cam.full_proj_transform
    px = int(round(((centre[0] / centre[3] + 1) * cam.image_width - 1) / 2))
    py = int(round(((centre[1] / centre[3] + 1) * cam.image_height - 1) / 2))
    from goi_hyperplane_amd import contrib
    seed = int(contrib.pick(tcam, pc, bg, (px, py)))
    assert 0 <= seed < P // 2, "the pixel is not over ball A"
    got = segment.pick(tcam, pc, bg, (px, py), seg).cpu().numpy()
    assert np.array_equal(np.flatnonzero(got), np.arange(P // 2))
    assert not segment.pick(tcam, pc, bg, (0, 0), seg).any()  # a corner of the image: nothing under it, nothing selected
