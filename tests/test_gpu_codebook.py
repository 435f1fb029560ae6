"""The code-book initialisation of csrc/codebook_init.hip on the GPU (semantic.unique_rows, spherical_kmeans,
init_codebook).

unique_rows equals torch.unique(dim=0) on the CPU exactly -- rows, order and count -- for few distinct rows, every row
distinct at >= 100 k pixels (the radix path), H * W not a multiple of 64, D in {16, 256, 512}, one pixel, +-0, half
precision, host and device input, and a batch equal to its views one at a time; NaN / Inf raise ValueError.
spherical_kmeans reproduces the reference's kmeans pins, agrees with io.kmeans on the device on well-separated data,
follows the zero-row, tie and raise rules, is bitwise reproducible, and batched equals one at a time.  init_codebook
reproduces the golden LUT of the reference stage and leaves the CPU generator in the same state."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import io as gio
from goi_hyperplane_amd import semantic
from tests.golden.make_codebook_golden import load_views

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def ref_unique(chw):
    return chw.cpu().float().permute(1, 2, 0).reshape(-1, chw.shape[0]).unique(dim=0)


def segment_map(D, H, W, segments, seed, zero=True):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(segments, D, generator=g)
    if zero:
        emb[0] = 0
    lab = torch.randint(0, segments, (H, W), generator=g)
    return emb[lab].permute(2, 0, 1).contiguous()


def check(maps):
    got = semantic.unique_rows(maps)
    lst = [maps] if torch.is_tensor(maps) else maps
    assert len(got) == len(lst)
    for m, u in zip(lst, got):
        ref = ref_unique(m)
        assert u.is_cuda and u.dtype == torch.float32
        assert u.shape == ref.shape
        assert torch.equal(u.cpu(), ref)
    return got


@pytest.mark.parametrize("D", [16, 256, 512])
def test_unique_rows_few_distinct(D):
    check(segment_map(D, 37, 53, 150, seed=D).cuda())  # 1961 pixels: not a multiple of 64


def test_unique_rows_every_row_distinct_radix_path():
    m = torch.randn(16, 320, 330)  # 105 600 distinct rows: the LSD radix path
    u = check(m.cuda())[0]
    assert u.shape[0] == 320 * 330


def test_unique_rows_distinct_rows_sharing_long_prefixes():
    g = torch.Generator().manual_seed(9)
    m = torch.zeros(16, 70, 90)
    m[15] = torch.randint(0, 3000, (70, 90), generator=g).float()  # rows differ only in the last channel
    m[3] = torch.randint(0, 2, (70, 90), generator=g).float() * -1.0
    check(m.cuda())


def test_unique_rows_one_pixel_and_signed_zeros():
    check(torch.randn(256, 1, 1).cuda())
    pm = torch.tensor([[0.0, -0.0, 0.0], [1.0, 1.0, -2.0]]).reshape(2, 1, 3).cuda()  # [0, 1] and [-0, 1] merge
    u = check(pm)[0]
    assert u.shape[0] == 2
    z = torch.tensor([0.0, -0.0]).reshape(1, 1, 2).cuda()
    assert check(z)[0].shape[0] == 1


def test_unique_rows_batch_equals_views_one_at_a_time_host_and_device():
    maps = [segment_map(64, 40, 50, 120, seed=s) for s in range(5)]
    one = [semantic.unique_rows(m.cuda())[0] for m in maps]
    dev = check([m.cuda() for m in maps])
    host = check(maps)
    for a, b, c in zip(one, dev, host):
        assert torch.equal(a, b) and torch.equal(a, c)
    mixed = semantic.unique_rows([maps[0], maps[1].cuda(), torch.randn(64, 8, 8)])  # different shapes, places
    assert torch.equal(mixed[0], one[0]) and torch.equal(mixed[1], one[1]) and mixed[2].shape == (64, 64)


def test_unique_rows_half_precision_is_exact():
    m = segment_map(32, 30, 40, 80, seed=4).half()
    u = semantic.unique_rows(m.cuda())[0]
    assert torch.equal(u.cpu(), ref_unique(m.float()))
    b = segment_map(32, 30, 40, 80, seed=5).bfloat16()
    assert torch.equal(semantic.unique_rows(b)[0].cpu(), ref_unique(b.float()))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_unique_rows_refuses_non_finite(bad):
    m = segment_map(16, 20, 20, 30, seed=1)
    m[7, 3, 4] = bad
    with pytest.raises(ValueError):
        semantic.unique_rows(m.cuda())


def test_spherical_kmeans_reproduces_the_reference_pins():
    z = np.load(os.path.join(GOLD, "ref_kmeans_pins.npz"))
    for name, k in (("k16", 16), ("k40_dead", 40)):
        x = torch.from_numpy(z["x"].copy()).cuda()
        torch.manual_seed(int(z["seed"]))
        c = semantic.spherical_kmeans(x, k)
        assert np.allclose(x.cpu().numpy(), z[name + "_x_after"], rtol=0, atol=1e-6)  # the norm sums in another order
        assert np.allclose(c.cpu().numpy(), z[name + "_centers"], rtol=0, atol=2e-6), name


def separated(n, d, centres, seed, noise=0.0):
    """n rows drawn from `centres` random directions.  With noise 0 the rows of a group are equal, so two centres seeded
    in one group are equal too and tie exactly (lowest index on both sides); with noise, a group split between two
    seeds is decided by the noise, and fp32 rounding in a different summation order can flip such a decision."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(centres, d, generator=g)
    return base[torch.randint(0, centres, (n,), generator=g)] + noise * torch.randn(n, d, generator=g)


@pytest.mark.parametrize("n,k", [(50, 8), (50, 80), (79, 80), (2000, 80), (2000, 300), (100000, 8), (100000, 80)])
def test_spherical_kmeans_agrees_with_io_kmeans_on_the_device(n, k):
    """Well separated for each k: up to 80 centres, rows repeat one of 400 random directions exactly (seeds in one group
    are equal centres and tie exactly: lowest index on both sides); at 300 centres -- where the library GEMM no longer
    gives equal columns bit-equal dot products -- every row is its own random direction in 256-d, and the best and
    second-best dot products stay far apart compared with fp32 rounding.  (At 100 000 rows x 300 centres random
    directions have best / second-best gaps below 1e-6, where a different summation order can flip a decision, so that
    size is covered by test_spherical_kmeans_is_reproducible_at_scale instead.)"""
    if k <= 80:
        x = separated(n, 64, 400, seed=n + k)
    else:
        x = torch.randn(n, 256, generator=torch.Generator().manual_seed(n + k))
    x = x.cuda()
    xa, xb = x.clone(), x.clone()
    torch.manual_seed(11)
    ref = gio.kmeans(xa, k)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    got = semantic.spherical_kmeans(xb, k)
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.allclose(xa, xb, rtol=0, atol=1e-6)
    assert torch.allclose(got, ref, rtol=0, atol=2e-6, equal_nan=True)


def test_spherical_kmeans_zero_rows_follow_the_nan_rule():
    x = torch.randn(400, 32, generator=torch.Generator().manual_seed(3))
    x[::7] = 0  # unlabelled pixels: NaN rows after normalisation, assigned to centre 0
    xa, xb = x.clone(), x.clone().cuda()
    torch.manual_seed(8)
    ref = gio.kmeans(xa, 12)
    torch.manual_seed(8)
    got = semantic.spherical_kmeans(xb, 12)
    assert torch.equal(xb.isnan().cpu(), xa.isnan())
    assert np.allclose(got.cpu().numpy(), ref.numpy(), rtol=0, atol=2e-6, equal_nan=True)


def test_spherical_kmeans_raises_where_the_reference_raises():
    x = separated(30, 16, 4, seed=2)
    torch.manual_seed(5)
    with pytest.raises(RuntimeError):
        gio.kmeans(x.clone(), 80)
    after_ref = torch.get_rng_state()
    torch.manual_seed(5)
    xb = x.clone().cuda()
    with pytest.raises(RuntimeError):
        semantic.spherical_kmeans(xb, 80)
    assert torch.equal(torch.get_rng_state(), after_ref)
    assert torch.allclose(xb.cpu(), x / x.norm(dim=1, keepdim=True), rtol=0, atol=1e-6)  # normalised before the raise


def test_spherical_kmeans_duplicate_centres_tie_to_the_lowest_index():
    """rows 6 and 7 equal row 0, and k = N: every permutation seeds three identical centres, whose dot products with
    every row are equal bit for bit; the lowest index takes the members and the other two die, as with torch's argmax"""
    x = torch.randn(6, 8, generator=torch.Generator().manual_seed(1))
    x = torch.cat([x, x[:1], x[:1]])
    for seed in range(4):
        torch.manual_seed(seed)
        ref = gio.kmeans(x.clone(), 8, niter=1)
        torch.manual_seed(seed)
        got = semantic.spherical_kmeans(x.clone().cuda(), 8, niter=1)
        assert np.allclose(got.cpu().numpy(), ref.numpy(), rtol=0, atol=2e-6), seed


def test_spherical_kmeans_is_reproducible_and_batched_equals_single():
    xs = [separated(n, 48, 60, seed=n, noise=0.05) for n in (150, 90, 2000, 33)]
    xs[0][:5] = 0
    torch.manual_seed(3)
    single = [semantic.spherical_kmeans(x.clone().cuda(), 40) for x in xs[:3]]
    state = torch.get_rng_state()
    torch.manual_seed(3)
    batched = semantic.spherical_kmeans_batched([x.clone().cuda() for x in xs[:3]], 40)
    assert torch.equal(torch.get_rng_state(), state)
    for a, b in zip(single, batched):
        assert torch.equal(a.nan_to_num(9.0), b.nan_to_num(9.0))
    torch.manual_seed(3)
    again = semantic.spherical_kmeans_batched([x.clone().cuda() for x in xs[:3]], 40)
    for a, b in zip(batched, again):
        assert torch.equal(a.nan_to_num(9.0), b.nan_to_num(9.0))
    torch.manual_seed(3)
    with pytest.raises(RuntimeError):  # 33 rows, 80 centres: the fourth problem raises like its own call
        semantic.spherical_kmeans_batched([x.clone().cuda() for x in xs], 80)


def test_spherical_kmeans_is_reproducible_at_scale():
    x = torch.randn(100000, 256, generator=torch.Generator().manual_seed(1)).cuda()
    torch.manual_seed(4)
    a = semantic.spherical_kmeans(x.clone(), 300)
    torch.manual_seed(4)
    b = semantic.spherical_kmeans(x.clone(), 300)
    assert a.shape == (300, 256) and torch.equal(a, b)
    assert not a.isnan().any()


def test_init_codebook_matches_the_golden_stage():
    z = np.load(os.path.join(GOLD, "ref_codebook_init_pins.npz"))
    views = load_views(z)
    maps = [m for m, _ in views]
    for (_, want), u in zip(views, semantic.unique_rows([m.cuda() for m in maps])):
        assert torch.equal(u.cpu(), want)
    torch.manual_seed(int(z["seed"]))
    lut = semantic.init_codebook(maps, tab_len=int(z["tab_len"]), per_view=int(z["per_view"]))
    assert lut.shape == z["lut"].shape and lut.dtype == torch.float32 and lut.is_cuda
    assert np.allclose(lut.cpu().numpy(), z["lut"], rtol=0, atol=2e-6, equal_nan=True)
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(z["rng_state"]))
