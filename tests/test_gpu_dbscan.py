"""Exact DBSCAN on the GPU (csrc/dbscan.hip through goi_semantic_dbscan): labels and core flags equal sklearn's on the
lattice pins of tests/golden/ref_dbscan_pins.npz and the numpy restatement (tests/dbscan_reference.py) on seeded sets up
to 200 k points; at 1 M points the core flags of a sample equal a brute-force count, two runs are bit-identical and a
permuted input gives the same partition.

Off the lattice the oracle is the restatement alone (exact fp32 fma), on the adversarial inputs of tests/dbscan_cases.py:
every case must give the restatement's labels, core flags and cluster count exactly, twice; the molecule and stack cases
must keep their labels under a scaling by 2^-30 and 2^30 and (molecules) their partition under a permutation; the ends of
the eps range and of the 2^21-cell axis limit are accepted with the right labels and refused one fp32 step further; a
strided view gives the labels of its copy.  No label differed: the +-2 window, the box prunes, the clique shortcut and the
two-word key sort hold on all of them.

What the cases hold (seed dbscan_cases.SEED; tests/test_dbscan_cases_cpu.py asserts the lower bounds).  bonds = pairs whose
d2 in the kernel's form is pred(eps2) / eps2 / succ(eps2); "bonds decided differently" = of those, the ones that the
unfused sum / the reversed fma order / float64 would decide the other way; "decisions wrong" = points whose core flag or
noise status changes when the brute force runs with that form (cases of <= 10 000 points; at min_samples 1 and on the
chain nothing is noise and every bond decided differently changes the cluster count by one instead).

  case                          n  clusters  noise  pred/ tie/succ   bonds decided differently   decisions wrong
  threshold_origin_ms1       4593      2773      0   868/ 952/ 899        704/ 953/ 934            (cluster count)
  threshold_origin_ms2       4593      1441   1332   868/ 952/ 899        704/ 953/ 934           1121/1469/1543
  threshold_origin_ms3       4593       379   3456   868/ 952/ 899        704/ 953/ 934            705/ 969/ 849
  threshold_offset_ms1       4269      2598      0   778/ 893/ 854        426/ 680/ 676            (cluster count)
  threshold_offset_ms2       4269      1339   1259   778/ 893/ 854        426/ 680/ 676            665/1031/1111
  threshold_offset_ms3       4269       332   3273   778/ 893/ 854        426/ 680/ 676            459/ 807/ 633
  threshold_small_eps_ms1    4663      2802      0   875/ 986/ 898        550/ 914/ 948            (cluster count)
  threshold_small_eps_ms2    4663      1472   1330   875/ 986/ 898        550/ 914/ 948            831/1411/1581
  threshold_small_eps_ms3    4663       389   3496   875/ 986/ 898        550/ 914/ 948            639/ 909/ 879
  threshold_large_eps_ms1    4537      2724      0   887/ 926/ 870        596/ 860/1138            (cluster count)
  threshold_large_eps_ms2    4537      1438   1286   887/ 926/ 870        596/ 860/1138            916/1325/1945
  threshold_large_eps_ms3    4537       375   3412   887/ 926/ 870        596/ 860/1138            612/ 933/ 987
  exact_ties_ms1             4000      3000      0     0/1000/   0     (every form is exact: tells <= from <)
  exact_ties_ms2             4000      1000   2000     0/1000/   0
  stacks_ms2                 1828       539    270   192/ 219/ 199        141/ 222/ 221            197/ 313/ 300
  stacks_ms64                4094        57    395    23/  23/  17         12/  22/  21            264/ 589/ 462
  stacks_ms65                3961        52    535    18/  19/  23         14/  19/  18            270/ 467/ 338
  stacks_ms257               7998        27   1035    12/   8/  11          7/  10/  10            519/ 522/ 522
  key_layout_ms1             2357      1469      0   423/ 465/ 461        182/ 324/ 348            (cluster count)
  key_layout_ms2             2357       732    737   423/ 465/ 461        182/ 324/ 348            300/ 518/ 593
  key_layout_ms3             2357       156   1889   423/ 465/ 461        182/ 324/ 348            174/ 330/ 291
  axis_limit                    4         2      0     1/   1/   0          2/   1/   1              4/   2/   2
  eps_limit_lo, eps_limit_hi    5         2      1     1/   1/   1          1/   2/   1              2/   3/   2
  chain                     21489        34      0    31/  32/  32         15/  27/  30            (cluster count)
  chain_short                5007        34      0    32/  31/  33         19/  28/  31            (cluster count)
  cloud_035_ms5_origin      10000         3   1125   clouds: blobs with noise as arbitrary floats, no constructed bonds
  cloud_035_ms10_far        30000         4   3183
  cloud_035_ms600_origin    20000         4   3722
  cloud_035_ms600_far       20000         4   3729
  cloud_002_ms5_far         10000         4   1136
  cloud_002_ms10_origin     30000         3   3193
  cloud_002_ms600_origin    20000         4   3652
  cloud_002_ms600_far       20000         4   3774
key_layout: 101 holding bonds have cy on either side of a multiple of 2^11, 567 have different cz, 130-136 points per axis
lie beyond cell 2^20.  chain: 33 breaks (32 succ(eps2) bonds and one step of eps that no nudge brought to a class), 34
clusters, 10 711 links with the key order and 10 683 against it, one cell per point.

Measured on an MI355X: the module's 101 tests take 24 s of wall time, 14 s of them the two large lattice sets of
test_equals_restatement (the host computes the restatement); every adversarial case takes under 0.7 s, restatement
included; the chain of 21 489 points takes 0.12 s (two device runs and the restatement: the parent walks of the
union-find are no burden at this length, so the chain was not shortened)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import dbscan_cases as dc
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


# ---- the adversarial cases of tests/dbscan_cases.py: decisions ON the threshold, off the lattice, at the grid's edges ----
@functools.lru_cache(maxsize=None)
def case_reference(name):
    return dbscan_reference(*dc.get(name))


def device_run(pts, eps, ms, dev):
    """(labels, core, cluster count) of one call, as device tensors."""
    from goi_hyperplane_amd.cluster import dbscan
    x = pts if torch.is_tensor(pts) else torch.tensor(pts, device=dev)
    labels, core = dbscan(x, eps, ms, return_core=True)
    return labels, core, dbscan.last_n_clusters


@pytest.mark.parametrize("name", list(dc.CASES))
def test_case_equals_restatement(name, dev):
    """Exact equality, no tolerance: labels, core flags and the cluster count, twice over."""
    pts, eps, ms = dc.get(name)
    want, want_core = case_reference(name)
    x = torch.tensor(pts, device=dev)
    labels, core, count = device_run(x, eps, ms, dev)
    labels2, core2, count2 = device_run(x, eps, ms, dev)
    assert torch.equal(labels, labels2) and torch.equal(core, core2) and count == count2
    np.testing.assert_array_equal(core.cpu().numpy(), want_core)
    np.testing.assert_array_equal(labels.cpu().numpy(), want)
    assert count == want.max() + 1


@pytest.mark.parametrize("name", dc.MOLECULE_CASES + dc.STACK_CASES)
def test_power_of_two_scaling_keeps_the_labels(name, dev):
    """dbscan(2^k X, 2^k eps) = dbscan(X, eps) for k = -30, 30: every operation of the form and of the grid scales exactly
    (tests/test_dbscan_cases_cpu.py shows that no square becomes subnormal).  With eps = 0.35 this reaches 2^-31.5 and
    2^28.5, towards both ends of the accepted range of eps."""
    pts, eps, ms = dc.get(name)
    labels, core, count = device_run(pts, eps, ms, dev)
    for k in (-30, 30):
        if not 2.0 ** -40 <= eps * 2.0 ** k <= 2.0 ** 40:  # (the eps-limit inputs already sit at an end of the range)
            continue
        got, got_core, got_count = device_run(np.ldexp(pts, k).astype(np.float32), float(np.ldexp(eps, k)), ms, dev)
        assert torch.equal(got_core, core) and torch.equal(got, labels) and got_count == count


def test_eps_range_ends(dev):
    """eps = 2^-40 and eps = 2^40 are accepted (test_case_equals_restatement[eps_limit_*] checks their labels); the next
    fp32 value outside is refused."""
    for name, outward in (("eps_limit_lo", 0.0), ("eps_limit_hi", np.inf)):
        pts, eps, ms = dc.get(name)
        assert eps in (2.0 ** -40, 2.0 ** 40)
        _, _, count = device_run(pts, eps, ms, dev)
        assert count == 2
        beyond = float(np.nextafter(np.float32(eps), np.float32(outward)))
        with pytest.raises(ValueError, match="2\\^21"):
            device_run(pts, beyond, ms, dev)


def test_axis_limit_is_one_fp32_step_wide(dev):
    """The last fp32 extent with fewer than 2^21 - 1 cells is clustered (the far pair sits in the last cells, where the +-2
    window is clamped: test_case_equals_restatement[axis_limit] checks the labels); one fp32 step more is refused."""
    pts, eps, ms = dc.get("axis_limit")
    labels, core, count = device_run(pts, eps, ms, dev)
    assert count == 2 and bool(core.all())
    for perm in ([0, 1, 2, 3], [3, 2, 1, 0]):
        over = dc.axis_limit(dc.SEED, over=True)[0][perm]
        with pytest.raises(ValueError, match="2\\^21"):
            device_run(np.ascontiguousarray(over), eps, ms, dev)
    # the limit is per axis: the same extent along y and along z (the form is not symmetric in the axes, so the rolled
    # input has labels of its own)
    for axis in (1, 2):
        roll = np.ascontiguousarray(np.roll(pts, axis, axis=1))
        want, want_core = dbscan_reference(roll, eps, ms)
        got, got_core, got_count = device_run(roll, eps, ms, dev)
        np.testing.assert_array_equal(got_core.cpu().numpy(), want_core)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert got_count == want.max() + 1
        with pytest.raises(ValueError, match="2\\^21"):
            device_run(np.ascontiguousarray(np.roll(dc.axis_limit(dc.SEED, over=True)[0], axis, axis=1)), eps, ms, dev)


@pytest.mark.parametrize("name", ["threshold_offset_ms2", "stacks_ms65", "key_layout_ms3"])
def test_strided_view_equals_contiguous_copy(name, dev):
    pts, eps, ms = dc.get(name)
    x = torch.tensor(pts, device=dev)
    wide = torch.full((len(pts), 8), float("nan"), device=dev)
    wide[:, 1:7:2] = x
    view = wide[:, 1:7:2]
    assert not view.is_contiguous() and view.stride() == (8, 2)
    labels, core, count = device_run(x, eps, ms, dev)
    got, got_core, got_count = device_run(view, eps, ms, dev)
    assert torch.equal(got, labels) and torch.equal(got_core, core) and got_count == count
    rows = torch.full((2 * len(pts), 3), float("nan"), device=dev)
    rows[::2] = x
    got, got_core, got_count = device_run(rows[::2], eps, ms, dev)
    assert torch.equal(got, labels) and torch.equal(got_core, core) and got_count == count


@pytest.mark.parametrize("name", dc.MOLECULE_CASES)
def test_permuted_case_gives_the_same_partition(name, dev):
    """What test_one_million_points asks of blobs, at the threshold: the same core set, the same noise set and a bijection
    between the two cluster numberings."""
    pts, eps, ms = dc.get(name)
    x = torch.tensor(pts, device=dev)
    labels, core, count = device_run(x, eps, ms, dev)
    perm = torch.from_numpy(np.random.default_rng(31).permutation(len(pts))).to(dev)
    lp, cp, count_p = device_run(x[perm], eps, ms, dev)
    assert torch.equal(cp, core[perm]) and torch.equal(lp == -1, labels[perm] == -1) and count_p == count
    keep = lp >= 0
    if bool(keep.any()):
        pairs = torch.unique(torch.stack([labels[perm][keep], lp[keep]]), dim=1)
        assert pairs.shape[1] == count  # every old number meets exactly one new number, and the reverse
        assert len(torch.unique(pairs[0])) == count == len(torch.unique(pairs[1]))
