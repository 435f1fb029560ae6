"""goi_hyperplane_amd.grouping on the GPU against its numpy restatement (tests/grouping_reference.py) on the cases of
tests/grouping_cases.py:
  1. count, qsum and qexp integer-equal, status 0; loss, intra, inter and grad within max(8 x the float32 twin's error against
     float64 on that case, 64 float32 ulps of the tensor's largest magnitude); an ignored pixel's gradient exactly 0;
  2. the same bits from two calls and from a call after unrelated work; qsum and count unchanged under a permutation of the
     pixels; backward with upstream 2 is 2 x the stored gradient bit for bit; without a gradient the loss has the same bits;
     nothing synchronises;
  3. end to end: two touching balls with ONE shared `_semantics` are one object to segment.instances and two after grouping.fit
     on eight views whose mask ids are swapped in every odd view.

The end-to-end fit runs FIT_ITERATIONS = 400 steps (the cap) of FusedAdam at FIT_LR = 0.02, margin 4, S = 16; both were found on
an MI355X, with the purity reached, and are in DESIGN.md 4.31 with the scenes on which the split is NOT reached.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import grouping
from tests import grouping_cases as gc
from tests import grouping_reference as ref

pytestmark = pytest.mark.gpu
ULPS = 64 * ref.EPS32
FLOATS = ("loss", "intra", "inter", "grad")
FIT_ITERATIONS, FIT_LR, FIT_MARGIN = 400, 0.02, 4.0
CHECKED = [n for n in gc.names() if n != "max_abs_exceeded"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def up(a):
    return torch.from_numpy(np.array(a)).to(torch.device("cuda:0"))  # (a copy: the cases are read-only)


def down(out):
    keys = ("loss", "intra", "inter", "grad", "count", "qsum", "qexp", "status")
    return {k: None if v is None else v.detach().cpu().numpy() for k, v in zip(keys, out)}


def run(c, want_grad=True, **over):
    f = up(c["feat"]).requires_grad_(want_grad)
    return grouping.loss_terms(f, up(c["labels"]), c["K"], **{**c["kw"], **over})


@functools.lru_cache(maxsize=None)
def on_device(name):
    return down(run(gc.case(name)))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHECKED)
def test_every_output_against_the_restatement(dev, name):
    c, got, want, twin = gc.case(name), on_device(name), gc.reference(name), gc.twin(name)
    S, H, W = c["feat"].shape
    assert got["count"].dtype == got["qsum"].dtype == np.int64 and got["count"].shape == (c["K"],) and got["qsum"].shape == (c["K"], S)
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["qsum"], want["qsum"])
    assert int(got["qexp"]) == want["qexp"] and int(got["status"]) == 0
    assert got["grad"].shape == (S, H, W) and got["grad"].dtype == got["loss"].dtype == np.float32
    for key in FLOATS:
        w64 = np.asarray(want[key], np.float64)
        e_twin = float(np.abs(np.asarray(twin[key], np.float64) - w64).max())
        tol = max(8 * e_twin, ULPS * float(np.abs(w64).max()))
        err = float(np.abs(got[key].astype(np.float64) - w64).max())
        print(f"{name} {key}: err {err:.3e} twin {e_twin:.3e} tol {tol:.3e}")
        assert err <= tol, (key, err, tol)
    ok = (c["labels"] >= 0) & (c["labels"] < c["K"])
    assert not bits(got["grad"])[:, ~ok].any(), "the gradient of an ignored pixel is +0"


def test_an_exceeded_max_abs_raises_bit_0(dev):
    assert int(on_device("max_abs_exceeded")["status"]) == 1


def test_max_abs_at_the_true_maximum_changes_no_bit(dev):
    c = gc.case("big_cells")
    given = down(run(c, max_abs=float(np.abs(c["feat"]).max())))
    for key, v in on_device("big_cells").items():
        assert np.array_equal(bits(given[key]), bits(v)), key


# ---- 2. the same bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big_cells", "tall_random64", "S3_K4096", "strips_2", "S32_K233"])
def test_two_calls_and_a_call_after_unrelated_work_give_the_same_bits(dev, name):
    first = on_device(name)
    again = down(run(gc.case(name)))
    noise = torch.randn(512, 512, device=dev)
    (noise @ noise).sum()
    third = down(run(gc.case(name)))
    for key, v in first.items():
        assert np.array_equal(bits(again[key]), bits(v)) and np.array_equal(bits(third[key]), bits(v)), key


@pytest.mark.parametrize("name", ["big_cells", "tall_random64"])
def test_the_integer_sums_do_not_depend_on_the_order_of_the_pixels(dev, name):
    c = gc.case(name)
    S, H, W = c["feat"].shape
    flat = dict(c, feat=c["feat"].reshape(S, 1, H * W), labels=c["labels"].reshape(1, H * W))
    perm = np.random.default_rng(5).permutation(H * W)
    moved = dict(c, feat=flat["feat"][:, :, perm], labels=flat["labels"][:, perm])
    a, b, base = down(run(flat)), down(run(moved)), on_device(name)
    for key in ("count", "qsum", "qexp"):
        assert np.array_equal(a[key], base[key]) and np.array_equal(b[key], base[key]), key


def test_backward_scales_the_stored_gradient_and_nothing_synchronises(dev):
    c = gc.case("big_cells")
    f, labels = up(c["feat"]).requires_grad_(True), up(c["labels"])
    plain = up(c["feat"])
    two = torch.tensor(2.0, device=dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = grouping.loss(f, labels, c["K"], **c["kw"])
        out.backward(two)
        alone = grouping.loss_terms(plain, labels, c["K"], **c["kw"])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    base = on_device("big_cells")
    assert out.dim() == 0 and out.dtype == torch.float32 and np.array_equal(bits(out.detach().cpu().numpy()), bits(base["loss"]))
    assert np.array_equal(bits(f.grad.cpu().numpy()), bits(2 * base["grad"]))
    assert alone[3] is None and not alone[0].requires_grad
    for key, v in zip(("loss", "intra", "inter"), alone[:3]):
        assert np.array_equal(bits(v.cpu().numpy()), bits(base[key])), key
    with torch.no_grad():
        assert grouping.loss_terms(f, labels, c["K"])[3] is None
    assert np.array_equal(plain.cpu().numpy(), c["feat"]) and np.array_equal(labels.cpu().numpy(), c["labels"])  # inputs untouched


def test_a_strided_feature_map_and_non_finite_features_terminate(dev):
    c = gc.case("small_ignored")
    wide = torch.zeros(32, 7, 20, device=dev)
    wide[:, :, 3:12] = up(c["feat"])
    got = down(grouping.loss_terms(wide[:, :, 3:12].requires_grad_(True), up(c["labels"]), c["K"]))
    for key, v in on_device("small_ignored").items():
        assert np.array_equal(bits(got[key]), bits(v)), key
    bad = c["feat"].copy()
    bad[0, 0, 3], bad[1, 2, 2] = np.nan, np.inf
    out = grouping.loss_terms(up(bad).requires_grad_(True), up(c["labels"]), c["K"])
    torch.cuda.synchronize()  # the caller's error: the numbers mean nothing, the call ends
    assert out[3].shape == (32, 7, 9)


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
def two_balls(dev):
    """Two touching balls of 1000 Gaussians each, as a mask generator's input shows objects: opaque (opacity 0.95) and made of
    Gaussians that are small beside them (sigma about 0.03 = 0.6 pixels, footprints of 2 pixels on balls 20 pixels across), so
    that "the ball of the pixel's dominant Gaussian" is a mask of what the pixel shows.  With sigma of a pixel and opacities of
    0.1 .. 0.9 every pixel near the contact, and every pixel of a view in which one ball shows through the other, blends both
    balls under one label; those views teach the Gaussians there a feature between the two means."""
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import make_camera, make_scene
    P, S = 2000, 16
    rng = np.random.default_rng(5)
    scene = make_scene(P, S=S, sh_degree=1, seed=3, log_scale_mean=-3.5)
    scene.opacities = np.full_like(scene.opacities, 0.95)
    u = rng.standard_normal((P, 3))
    inside = u / np.linalg.norm(u, axis=1, keepdims=True) * (0.5 * rng.random((P, 1)) ** (1 / 3))  # uniform in a ball of radius 0.5
    ball = (np.arange(P) >= P // 2).astype(np.int64)  # ball A around (-0.5, 0, 0), ball B around (+0.5, 0, 0): they touch
    scene.means3D = (inside + np.stack([ball - 0.5, 0 * ball, 0 * ball], 1)).astype(np.float32)
    scene.semantics = (np.eye(S)[0][None, :] + 0.01 * rng.standard_normal((P, S))).astype(np.float32)  # ONE feature for both
    pc = GaussianSet.from_scene(scene, dev)
    cams = [TorchCamera(make_camera(64, 64, yaw=2 * np.pi * i / 8, pitch=0.3, distance=3.0), dev) for i in range(8)]
    return pc, cams, torch.from_numpy(ball).to(dev)


def label_maps(pc, cams, ball, dev):
    """each view's map: the ball of the pixel's dominant Gaussian, -1 for the background; the two ids swapped in every odd view"""
    from goi_hyperplane_amd import contrib
    black = torch.zeros(3, device=dev)
    maps = []
    for i, cam in enumerate(cams):
        top = contrib.frame(cam, pc, black).top_id.long()
        own = ball[top.clamp(min=0)]
        if i & 1:
            own = 1 - own
        maps.append(torch.where(top >= 0, own, torch.full_like(own, -1)).to(torch.int32))
    return maps


def fit_two_balls(dev, iterations=FIT_ITERATIONS, lr=FIT_LR, **kw):
    from goi_hyperplane_amd import contrib
    pc, cams, ball = two_balls(dev)
    maps = label_maps(pc, cams, ball, dev)
    features = grouping.fit(cams, pc, maps, 2, S=16, iterations=iterations, lr=lr, seed=0, **{**dict(margin=FIT_MARGIN), **kw})
    seen = contrib.peak_weights(cams, pc, torch.zeros(3, device=dev)) > 0
    seg = grouping.instances(pc.get_xyz.detach(), features, seen, tau=kw.get("margin", FIT_MARGIN) / 2)
    return pc, ball, maps, features, seen, seg


def purity(ball, seen, seg):
    """-> (share of the seen Gaussians in the two largest instances, the larger share of foreign seen members among the two)"""
    label = seg.label.cpu().numpy()
    seen, ball = seen.cpu().numpy(), ball.cpu().numpy()
    ids, sizes = np.unique(label[seen & (label >= 0)], return_counts=True)
    top = ids[np.argsort(-sizes, kind="stable")[:2]]
    held = sum(int((seen & (label == k)).sum()) for k in top) / max(int(seen.sum()), 1)
    foreign = 0.0
    for k in top:
        mine = ball[seen & (label == k)]
        foreign = max(foreign, 1.0 - np.bincount(mine, minlength=2).max() / max(mine.size, 1))
    return held, foreign, len(top)


@functools.lru_cache(maxsize=None)
def fitted():
    return fit_two_balls(torch.device("cuda:0"))


def test_one_semantic_feature_gives_one_object_and_the_fit_repeats_bit_for_bit(dev):
    from goi_hyperplane_amd import segment
    pc, ball, maps, features, seen, seg = fitted()
    # why the feature exists: on `_semantics` the two balls are one object
    whole = segment.instances(pc.get_xyz.detach(), pc._semantics.detach(), k=8, tau=0.5)
    assert whole.count.cpu().tolist() == [1]
    assert all(m.dtype == torch.int32 and set(m.unique().cpu().tolist()) == {-1, 0, 1} for m in maps)
    assert features.shape == (2000, 16) and features.dtype == torch.float32 and not features.requires_grad
    assert bool(torch.isfinite(features).all()) and float(features.abs().max()) > 0.5  # it moved, and stayed finite
    again = fit_two_balls(dev)
    assert torch.equal(again[3], features) and torch.equal(again[5].label, seg.label), "the same seed gives the same bits"


def test_two_touching_balls_with_one_semantic_feature_become_two_instances(dev):
    """The conditions of the feature's issue: the two largest instances hold at least 90 % of the seen Gaussians and neither has
    5 % or more of its seen members from the other ball, at tau = margin / 2.  Measured on an MI355X with this scene and fit
    (400 iterations, lr 0.02, margin 4): 1931 of 2000 Gaussians seen, the two largest instances hold 95.8 %, foreign share 1.2 %;
    with segment's mutual=True 94.5 % / 0.0 %, with k = 4 93.9 % / 0.0 %; from a camera distance of 2.4 instead of 3: 96.5 % / 0.3 %."""
    pc, ball, maps, features, seen, seg = fitted()
    held, foreign, n = purity(ball, seen, seg)
    print(f"two balls: {int(seen.sum())} seen, the two largest instances hold {held:.4f}, foreign share {foreign:.4f}")
    assert n == 2 and held >= 0.90
    assert foreign < 0.05
