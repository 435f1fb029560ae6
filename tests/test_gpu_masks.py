"""The mask kernels of csrc/masks.hip on the GPU (goi_hyperplane_amd/masks.py).

pack: the bits equal sim > 0 and the two counts equal count_nonzero and (sim > 0).sum(), with NaN, negative similarities,
widths that are not multiples of 64 and H = 1.  dilate: equals the clipped-window restatement (tests/mask_reference.py),
at three frame sizes, densities from 0.1 % to 50 %, empty and full masks, single pixels in the corners and radii 0 to 63,
and F.max_pool2d as a further cross-check; a batch in one launch equals its views done one at a time.  confusion and
segmentation_metrics: equal torch and the reference metrics pinned in tests/golden/ref_mask_metric_pins.npz.  The mask
stage on maps already rendered runs under torch.cuda.set_sync_debug_mode("error")."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.mask_reference import confusion_reference, dilate_reference

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def unpacked_bits(packed, W):
    """Host view of a packed buffer: bool [V, H, W] from the uint64 words (little-endian bit order within a word)."""
    a = packed.cpu().numpy().view(np.uint64)
    bits = (a[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    full = bits.reshape(a.shape[0], a.shape[1], -1).astype(bool)
    assert not full[..., W:].any(), "bits past W must be zero"
    return full[..., :W]


@pytest.mark.parametrize("W", [1, 63, 64, 65, 511, 800, 1600])
@pytest.mark.parametrize("H", [1, 37])
def test_pack_bits_and_counts(dev, H, W):
    from goi_hyperplane_amd import masks
    g = torch.Generator(device=dev).manual_seed(H * 10007 + W)
    sim = torch.rand((3, H, W), generator=g, device=dev) * 2 - 0.6  # negative, zero and positive similarities
    sim[sim.abs() < 0.2] = 0.0
    sim[0].view(-1)[:: 7] = float("nan")
    sim[1].view(-1)[1:: 11] = -float("nan")
    packed, counts = masks.pack(sim)
    assert packed.shape == (3, H, masks.words(W)) and packed.dtype == torch.int64
    want = (sim > 0).cpu().numpy()
    assert np.array_equal(unpacked_bits(packed, W), want)
    want_counts = torch.stack([torch.count_nonzero(sim.reshape(3, -1), dim=1), (sim > 0).reshape(3, -1).sum(1)], 1)
    assert torch.equal(counts, want_counts)
    assert torch.equal(masks.unpack(packed, W), (sim > 0).unsqueeze(1))
    # bool and uint8 masks: x != 0
    m8 = (sim > 0.1).to(torch.uint8) * 3
    p8, c8 = masks.pack(m8)
    assert np.array_equal(unpacked_bits(p8, W), (m8 != 0).cpu().numpy())
    assert torch.equal(c8[:, 0], c8[:, 1]) and torch.equal(c8[:, 0], (m8 != 0).reshape(3, -1).sum(1))
    pb, _ = masks.pack(m8 != 0)
    assert torch.equal(pb, p8)


def test_pack_into_slots(dev):
    from goi_hyperplane_amd import masks
    H, W, V = 40, 130, 5
    maps = torch.randn((V, H, W), device=dev)
    packed = torch.full((V, H, masks.words(W)), -1, dtype=torch.int64, device=dev)
    counts = torch.zeros((V, 2), dtype=torch.int64, device=dev)
    for v in (3, 0, 4, 1, 2):
        masks.pack_into(maps[v], packed, counts, v)
    ref, ref_counts = masks.pack(maps)
    assert torch.equal(packed, ref) and torch.equal(counts, ref_counts)
    with pytest.raises(ValueError):
        masks.pack_into(maps[0], packed, counts, V)


SHAPES = [(512, 512), (528, 800), (1056, 1600)]


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("density", [0.001, 0.01, 0.1, 0.5])
def test_dilate_equals_the_window_definition(dev, H, W, density):
    from goi_hyperplane_amd import masks
    rng = np.random.default_rng(int(density * 1000) + W)
    m = rng.random((H, W)) < density
    got = masks.dilate(torch.from_numpy(m).to(dev), 3, 5)
    assert got.dtype == torch.bool and got.shape == (H, W)
    assert np.array_equal(got.cpu().numpy(), dilate_reference(m, 5))
    pool = F.max_pool2d(torch.from_numpy(m).to(dev).float()[None, None], 11, 1, 5)[0, 0] > 0
    assert torch.equal(got, pool)


@pytest.mark.parametrize("r", [0, 1, 5, 31, 63])
def test_dilate_radii_corners_empty_full(dev, r):
    from goi_hyperplane_amd import masks
    H, W = 528, 800
    m = np.zeros((4, H, W), bool)
    m[0, 0, 0] = m[0, 0, W - 1] = m[0, H - 1, 0] = m[0, H - 1, W - 1] = True  # the four corners
    m[1, 100, 63] = m[1, 200, 64] = m[1, 300, 127] = m[1, 301, 128] = m[1, 5, 799] = True  # word edges
    m[3] = True
    rng = np.random.default_rng(r)
    extra = rng.random((H, W)) < 0.002
    k, n = (1, 1) if r == 0 else (2 * r + 1, 1)
    got = masks.dilate(torch.from_numpy(m).to(dev), k, n).cpu().numpy()
    for v in range(4):
        assert np.array_equal(got[v], dilate_reference(m[v], r)), v
    assert not got[2].any() and got[3].all()
    if r:
        got2 = masks.dilate(torch.from_numpy(extra).to(dev), 3, r).cpu().numpy()  # the same radius as iterations of 3x3
        assert np.array_equal(got2, dilate_reference(extra, r))


def test_dilate_batch_equals_views_one_at_a_time(dev):
    from goi_hyperplane_amd import masks
    V, H, W = 6, 257, 333
    rng = np.random.default_rng(7)
    m = torch.from_numpy(rng.random((V, H, W)) < np.linspace(0.001, 0.4, V)[:, None, None]).to(dev)
    packed, _ = masks.pack(m)
    batch = masks.dilate_packed(packed, W, 5)
    for v in range(V):
        one = masks.dilate_packed(masks.pack(m[v])[0], W, 5)
        assert torch.equal(batch[v], one[0]), v
    assert torch.equal(masks.unpack(batch, W)[:, 0], masks.dilate(m))
    # a uint8 mask gives the same, and the leading dimensions are kept
    assert torch.equal(masks.dilate(m.to(torch.uint8).reshape(2, 3, H, W)), masks.dilate(m).reshape(2, 3, H, W))


def test_unpack_selected_views(dev):
    from goi_hyperplane_amd import masks
    m = torch.rand((7, 33, 70), device=dev) > 0.5
    packed, _ = masks.pack(m)
    idx = torch.tensor([5, 0, 3], device=dev)
    assert torch.equal(masks.unpack(packed, 70, idx), m[idx].unsqueeze(1))
    assert masks.unpack(packed, 70, idx[:0]).shape == (0, 1, 33, 70)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 65), (48, 80), (512, 512), (1056, 1600)])
def test_confusion_equals_torch(dev, H, W):
    from goi_hyperplane_amd import masks
    g = torch.Generator(device=dev).manual_seed(H + W)
    pred = torch.rand((4, H, W), generator=g, device=dev) - 0.7
    gt = torch.rand((4, H, W), generator=g, device=dev) > 0.5
    gt[1] = False
    gt[2] = True
    got = masks.confusion(pred, gt)
    p = pred > 0
    want = torch.stack([(p & gt).reshape(4, -1).sum(1), (p & ~gt).reshape(4, -1).sum(1), (~p & gt).reshape(4, -1).sum(1),
                        (~p & ~gt).reshape(4, -1).sum(1)], 1)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert int(got.sum()) == 4 * H * W


def test_confusion_and_metrics_equal_the_pins(dev):
    from goi_hyperplane_amd import masks
    pins = np.load(os.path.join(GOLD, "ref_mask_metric_pins.npz"))
    for name in (str(n) for n in pins["cases"]):
        shape = tuple(int(v) for v in pins[f"{name}_shape"])
        n = shape[0] * shape[1]
        pred = np.unpackbits(pins[f"{name}_pred"], count=n).astype(bool).reshape(shape)
        gt = np.unpackbits(pins[f"{name}_gt"], count=n).astype(bool).reshape(shape)
        c = masks.confusion(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev))
        assert np.array_equal(c.cpu().numpy()[0], confusion_reference(pred, gt)), name
        m = masks.segmentation_metrics(c)
        for got, key in ((m.iou, "iou"), (m.mpa, "mpa"), (m.mp, "mp")):
            want = pins[f"{name}_{key}"]
            assert got[0].numpy().dtype == want.dtype and got[0].numpy().tobytes() == want.tobytes(), (name, key)


def test_mask_stage_does_not_synchronise(dev):
    from goi_hyperplane_amd import masks
    V, H, W = 8, 512, 512
    sims = torch.randn((V, H, W), device=dev)
    gt = torch.rand((V, H, W), device=dev) > 0.5
    keep_idx = torch.tensor([1, 4, 6], device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        packed = torch.empty((V, H, masks.words(W)), dtype=torch.int64, device=dev)
        counts = torch.zeros((V, 2), dtype=torch.int64, device=dev)
        for v in range(V):
            masks.pack_into(sims[v], packed, counts, v)
        dilated = masks.dilate_packed(packed, W, 5)
        sem = masks.unpack(packed, W, keep_idx)
        semd = masks.unpack(dilated, W, keep_idx)
        gtp, _ = masks.pack(gt)
        conf = masks.confusion_packed(packed, gtp, W)
        d = masks.dilate(gt)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(sem[:, 0], sims[keep_idx] > 0)
    assert np.array_equal(semd[1, 0].cpu().numpy(), dilate_reference((sims[4] > 0).cpu().numpy(), 5))
    assert torch.equal(counts[:, 0], torch.count_nonzero(sims.reshape(V, -1), dim=1))
    assert int(conf.sum()) == V * H * W and d.shape == gt.shape
