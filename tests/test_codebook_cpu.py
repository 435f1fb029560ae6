"""CPU checks of the code-book initialisation contract (csrc/codebook_init.hip, semantic.init_codebook).

* k-means with its permutations drawn up front (tests/codebook_reference.py) equals io.kmeans -- pinned to the
  reference's own function -- bit for bit, for N > k, N < k, zero rows, and the shape-mismatch raise, and leaves the
  generator where io.kmeans leaves it.
* the kernel's order-preserving keys order rows as torch.unique(dim=0) on the CPU does, with +-0 merged.
* the golden pins (tests/golden/ref_codebook_init_pins.npz, from the reference's kmeans) are reproduced by the
  restatements."""
import os

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import io as gio
from tests.codebook_reference import draw_perms, kmeans_preperm, unique_rows_by_keys
from tests.golden.make_codebook_golden import load_views

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_codebook_init_pins.npz")


def separated(n, d, centres, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(centres, d, generator=g)
    return base[torch.randint(0, centres, (n,), generator=g)] + 0.05 * torch.randn(n, d, generator=g)


@pytest.mark.parametrize("n,k,zeros", [(900, 16, 0), (200, 40, 0), (79, 80, 0), (50, 80, 0), (300, 24, 7), (2, 3, 0)])
def test_preperm_kmeans_equals_io_kmeans_bit_for_bit(n, k, zeros):
    x = separated(n, 32, 12, seed=n + k)
    x[:zeros] = 0
    xa, xb = x.clone(), x.clone()
    torch.manual_seed(77)
    ref = gio.kmeans(xa, k)
    after_ref = torch.get_rng_state()
    torch.manual_seed(77)
    got = kmeans_preperm(xb, k, 10, draw_perms(n, 10))
    assert torch.equal(torch.get_rng_state(), after_ref)
    assert torch.equal(xa.nan_to_num(7.0), xb.nan_to_num(7.0))
    assert torch.equal(ref.nan_to_num(7.0), got.nan_to_num(7.0))


def test_preperm_kmeans_raises_where_io_kmeans_raises():
    x = separated(30, 16, 4, seed=3)
    torch.manual_seed(5)
    with pytest.raises(RuntimeError):
        gio.kmeans(x.clone(), 80)
    with pytest.raises(RuntimeError):
        kmeans_preperm(x.clone(), 80, 10, draw_perms(30, 10))


def test_order_keys_sort_like_torch_unique():
    g = torch.Generator().manual_seed(2)
    vals = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.5, -2.5, 1e-30, -1e-30, 3e38, -3e38])
    rows = vals[torch.randint(0, len(vals), (4000, 3), generator=g)]
    chw = rows.T.reshape(3, 40, 100).contiguous()
    ref = chw.permute(1, 2, 0).reshape(-1, 3).unique(dim=0)
    got = unique_rows_by_keys(chw)
    assert torch.equal(ref, got)  # values compare equal: -0 == 0
    pm = torch.tensor([[0.0, -0.0], [1.0, 1.0]]).reshape(2, 1, 2)  # rows [0, 1] and [-0, 1]
    assert pm.permute(1, 2, 0).reshape(-1, 2).unique(dim=0).shape[0] == 1
    assert unique_rows_by_keys(pm).shape[0] == 1


def test_golden_pins_are_reproduced_by_the_restatements():
    z = np.load(GOLD)
    torch.manual_seed(int(z["seed"]))
    tots = []
    for m, want in load_views(z):
        assert torch.equal(m.permute(1, 2, 0).reshape(-1, m.shape[0]).unique(dim=0), want)  # what the pins stored
        u = unique_rows_by_keys(m)
        assert torch.equal(u, want)
        tots.append(kmeans_preperm(u.clone(), int(z["per_view"]), 10, draw_perms(u.shape[0], 10)))
    tot = torch.cat(tots, 0)
    assert np.allclose(tot.numpy(), z["tot"], rtol=0, atol=2e-6, equal_nan=True)
    lut = kmeans_preperm(tot, int(z["tab_len"]), 10, draw_perms(tot.shape[0], 10)).float()
    assert np.allclose(lut.numpy(), z["lut"], rtol=0, atol=2e-6, equal_nan=True)
    assert torch.equal(torch.get_rng_state(), torch.from_numpy(z["rng_state"]))
