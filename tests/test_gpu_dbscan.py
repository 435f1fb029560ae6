"""Exact DBSCAN on the GPU (csrc/dbscan.hip through goi_semantic_dbscan): labels and core flags equal sklearn's on the
lattice pins of tests/golden/ref_dbscan_pins.npz and the numpy restatement (tests/dbscan_reference.py) on seeded sets up
to 200 k points; at 1 M points the core flags of a sample equal a brute-force count, two runs are bit-identical and a
permuted input gives the same partition."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests.dbscan_reference import dbscan_reference, lattice_blobs
from tests.test_dbscan_cpu import pin_case, pins  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PIN_CASES = ["blobs600", "blobs10", "border_border_first", "border_border_last", "border_b_first", "border_mixed",
             "duplicates", "min_samples_1", "min_samples_gt_n", "far_extent", "n1"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def run(pts, eps, ms, dev):
    from goi_hyperplane_amd.cluster import dbscan
    labels, core = dbscan(torch.from_numpy(np.ascontiguousarray(pts)).to(dev), eps, ms, return_core=True)
    return labels.cpu().numpy(), core.cpu().numpy()


@pytest.mark.parametrize("name", PIN_CASES)
def test_equals_sklearn_pins(pins, name, dev):  # noqa: F811
    from goi_hyperplane_amd.cluster import dbscan
    pts, eps, ms, labels, core = pin_case(pins, name)
    got, got_core = run(pts, eps, ms, dev)
    np.testing.assert_array_equal(got_core, core)
    np.testing.assert_array_equal(got, labels)
    assert dbscan.last_n_clusters == labels.max() + 1


@pytest.mark.parametrize("n,ms,seed,spread", [(1000, 5, 1, 0.3), (20000, 10, 2, 0.5), (50000, 600, 3, 0.3),
                                               (200000, 600, 4, 0.6)])
def test_equals_restatement(n, ms, seed, spread, dev):
    pts = lattice_blobs(np.random.default_rng(seed), n, spread=spread)
    want, want_core = dbscan_reference(pts, 0.35, ms)
    got, got_core = run(pts, 0.35, ms, dev)
    np.testing.assert_array_equal(got_core, want_core)
    np.testing.assert_array_equal(got, want)


def _brute_core(x, q, eps, ms):
    """Neighbour counts of the query rows q against all of x in the kernel's fp32 form (fma as one rounding of the exact
    float64 value: exact on the lattice)."""
    eps2 = torch.tensor(np.float32(np.float32(eps) * np.float32(eps)), device=x.device)
    cnt = []
    for s in range(0, q.shape[0], 16):
        d = q[s:s + 16, None, :] - x[None]
        t = (d[..., 1].double() * d[..., 1].double() + (d[..., 0] * d[..., 0]).double()).float()
        d2 = (d[..., 2].double() * d[..., 2].double() + t.double()).float()
        cnt.append((d2 <= eps2).sum(1))
    return torch.cat(cnt) >= ms


def test_one_million_points(dev):
    from goi_hyperplane_amd.cluster import dbscan
    n = 1_000_000
    pts = lattice_blobs(np.random.default_rng(11), n, centers=6, spread=0.8, extent=6.0)
    x = torch.from_numpy(pts).to(dev)
    labels, core = dbscan(x, 0.35, 600, return_core=True)
    labels2, core2 = dbscan(x, 0.35, 600, return_core=True)
    assert torch.equal(labels, labels2) and torch.equal(core, core2)  # bit-identical from run to run
    assert 0 < int(core.sum()) < n and int(labels.max()) >= 0
    sample = torch.from_numpy(np.random.default_rng(12).choice(n, 2000, replace=False)).to(dev)
    assert torch.equal(core[sample], _brute_core(x, x[sample], 0.35, 600))
    # a permuted input: the same core set, the same noise set, the same partition of the core points
    perm = torch.from_numpy(np.random.default_rng(13).permutation(n)).to(dev)
    lp, cp = dbscan(x[perm], 0.35, 600, return_core=True)
    assert torch.equal(cp, core[perm])
    assert torch.equal(lp == -1, labels[perm] == -1)
    a, b = labels[perm][cp], lp[cp]
    pairs = torch.unique(torch.stack([a, b]), dim=1)
    assert pairs.shape[1] == int(a.max()) + 1 == int(b.max()) + 1  # a bijection between the two numberings


def test_numpy_in_numpy_out(pins, dev):  # noqa: F811
    from goi_hyperplane_amd.cluster import DBSCAN
    pts, eps, ms, labels, core = pin_case(pins, "blobs10")
    db = DBSCAN(eps=eps, min_samples=ms)
    out = db.fit_predict(pts)
    assert isinstance(out, np.ndarray) and out.dtype == np.int64
    np.testing.assert_array_equal(out, labels)
    np.testing.assert_array_equal(db.core_sample_indices_, np.nonzero(core)[0])
    t = DBSCAN(eps=eps, min_samples=ms).fit(torch.from_numpy(pts).to(dev))
    assert torch.is_tensor(t.labels_) and t.labels_.is_cuda and t.labels_.dtype == torch.int64
    np.testing.assert_array_equal(t.labels_.cpu().numpy(), labels)


def test_non_finite_and_empty_and_range(dev):
    from goi_hyperplane_amd.cluster import dbscan
    x = torch.rand(1000, 3, device=dev)
    x[17, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        dbscan(x, 0.35, 5)
    x[17, 1] = float("inf")
    with pytest.raises(ValueError, match="infinity"):
        dbscan(x, 0.35, 5)
    empty = dbscan(torch.zeros(0, 3, device=dev), 0.35, 5)
    assert empty.shape == (0,) and dbscan.last_n_clusters == 0
    far = torch.tensor([[0.0, 0.0, 0.0], [1e6, 0.0, 0.0]], device=dev)  # 2^21 cells of eps / sqrt(3) do not span it
    with pytest.raises(ValueError, match="2\\^21"):
        dbscan(far, 0.35, 1)
    ok = dbscan(torch.tensor([[0.0, 0.0, 0.0], [1e4, 0.0, 0.0]], device=dev), 0.35, 1)
    assert ok.tolist() == [0, 1]
