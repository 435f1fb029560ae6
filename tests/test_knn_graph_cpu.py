"""The k-NN graph without a GPU: the numpy restatement (tests/knn_graph_reference.py) against the distCUDA2 oracle and a float64
k-d tree, its label and padding rules, and what the three C entries declare, export and refuse before any device call."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
from scipy.spatial import cKDTree

from oracle import oracle
from tests import knn_graph_reference as ref
from tests.test_knn_cpu import clouds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
MIS = C.c_void_p((1 << 20) + 4)
N = None
TIE_FREE = ["gauss_aniso", "clusters", "positive_octant", "box_edge_1025"]


@functools.lru_cache(maxsize=None)
def rows17(name):
    """the reference's 17 nearest others of every point of a cloud (k <= 16 rows are its prefixes), computed once"""
    pts = clouds()[name]
    return ref.knn_rows(pts, pts, 17, exclude_self=True)


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", list(clouds()))
def test_k3_rows_give_the_dist2_oracle_bit_for_bit(name):
    pts = clouds()[name]
    _, d = rows17(name)
    mean = ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3)
    assert mean.dtype == np.float32
    assert np.array_equal(mean, oracle.knn_mean_dist2(pts, fma=True)), name


@pytest.mark.parametrize("name", list(clouds()))
def test_rows_are_prefixes_and_ordered(name):
    pts = clouds()[name][:700]
    i17, d17 = ref.knn_rows(pts, pts, 16, exclude_self=True)
    for k in (1, 3, 8):
        i, d = ref.knn_rows(pts, pts, k, exclude_self=True)
        assert np.array_equal(i, i17[:, :k]) and np.array_equal(d, d17[:, :k])
    assert np.all((d17[:, 1:] > d17[:, :-1]) | ((d17[:, 1:] == d17[:, :-1]) & (i17[:, 1:] > i17[:, :-1])))
    assert not np.any(i17 == np.arange(len(pts))[:, None])


def test_dist2_is_symmetric_bitwise():
    for name, pts in clouds().items():
        d = ref.dist2_matrix(pts[:400], pts[:400])
        assert np.array_equal(d, d.T), name


def test_fused_arithmetic_undoes_double_rounding():
    """a * a + b whose float64 sum lands exactly on an fp32 midpoint although the exact value does not"""
    a = np.array([1.0 + 2.0 ** -12], np.float32)  # a * a = 1 + 2^-11 + 2^-24: the fp32 midpoint between 1 + 2^-11 and the next
    b = np.array([2.0 ** -60], np.float32)        # lost by the float64 sum; the exact value is above the midpoint
    assert ref._fma_sq(a, b)[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert (a.astype(np.float64) * a + b.astype(np.float64)).astype(np.float32)[0] == np.float32(1 + 2.0 ** -11)  # round-to-even: wrong


@pytest.mark.parametrize("name", TIE_FREE)
@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_neighbour_sets_against_float64_kdtree(name, k):
    pts = clouds()[name]
    p64 = pts.astype(np.float64)
    d, j = cKDTree(p64).query(p64, k=k + 2)  # self, then k + 1 others
    d2 = d[:, 1:] ** 2
    near_tie = np.any(np.diff(d2, axis=1) < 2e-6 * d2[:, 1:], axis=1)
    left_out = near_tie.mean()
    print(f"{name} k={k}: {100 * left_out:.3f} % of rows are near-ties")
    assert left_out <= 0.005
    got = np.sort(rows17(name)[0][:, :k], axis=1)
    want = np.sort(j[:, 1:k + 1], axis=1)
    assert np.array_equal(got[~near_tie], want[~near_tie])


def test_majority_tie_rule_cut_and_padding():
    labels = np.array([5, 2, 2, 5, -1, 9], np.int64)
    idx = np.array([[0, 1, 2, 3],      # 5, 2, 2, 5: a tie -> the lowest, 2
                    [0, 3, 1, 4],      # 5, 5, 2, unlabelled -> 5
                    [4, 4, -1, -1],    # nothing admissible
                    [5, -1, -1, -1],   # padding ignored
                    [1, 0, 3, 5]], np.int32)
    lab, cnt = ref.majority_labels(idx, labels)
    assert lab.tolist() == [2, 5, -1, 9, 5] and cnt.tolist() == [2, 2, 0, 1, 2]
    dist2 = np.array([[1, 2, 3, 4], [1, 2, 3, 4], [1, 1, np.inf, np.inf], [7, np.inf, np.inf, np.inf], [1, 2, 2.5, 3]], np.float32)
    lab, cnt = ref.majority_labels(idx, labels, dist2, 2.0)  # <= : the entry AT the cut counts
    assert lab.tolist() == [2, 5, -1, -1, 2] and cnt.tolist() == [1, 2, 0, 0, 1]
    lab, cnt = ref.majority_labels(idx, labels, dist2, np.inf)
    assert lab.tolist() == [2, 5, -1, 9, 5]


def test_rows_are_padded_where_references_run_out():
    pts = clouds()["gauss_aniso"][:5]
    i, d = ref.knn_rows(pts, pts, 8, exclude_self=True)
    assert np.all(i[:, :4] >= 0) and np.all(i[:, 4:] == -1) and np.all(np.isinf(d[:, 4:])) and np.all(np.isfinite(d[:, :4]))
    keep = np.array([1, 0, 1, 0, 0], bool)
    i, d = ref.knn_rows(pts, pts, 2, query_keep=keep, ref_keep=keep, exclude_self=True)
    assert i.tolist() == [[2, -1], [-1, -1], [0, -1], [-1, -1], [-1, -1]]
    i, d = ref.knn_rows(pts, pts[:0], 3)
    assert np.all(i == -1) and np.all(np.isinf(d)) and i.shape == (5, 3)


def test_complete_labels_edges():
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((300, 3)).astype(np.float32)
    full = rng.integers(0, 4, 300)
    assert np.array_equal(ref.complete_labels(pts, full), full)  # all labelled: unchanged
    none = np.full(300, -1, np.int64)
    assert np.array_equal(ref.complete_labels(pts, none), none)  # nobody to learn from
    part = np.where(rng.random(300) < 0.3, full, -1)
    assert np.array_equal(ref.complete_labels(pts, part, selection=np.zeros(300, bool)), part)  # none in selection
    done = ref.complete_labels(pts, part, k=3)
    assert np.all(done >= 0) and np.array_equal(done[part >= 0], part[part >= 0])
    sel = rng.random(300) < 0.5
    half = ref.complete_labels(pts, part, k=3, selection=sel)
    assert np.array_equal(half[~sel], part[~sel]) and np.all(half[sel] >= 0)


def test_entries_are_declared_and_exported(lib):
    from goi_hyperplane_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    for name in ("goi_knn_graph_workspace_bytes", "goi_knn_graph", "goi_knn_majority"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert name in hdr.split("#define GOI_RASTER_ABI_VERSION")[0], f"{name} is not in the list of later additions"
    assert lib.goi_raster_abi_version() == _lib.ABI_VERSION == 9


def test_workspace_size(lib):
    size = lib.goi_knn_graph_workspace_bytes
    for bad in ((-1, 10), (10, -1), (2 ** 30, 10), (10, 2 ** 30)):
        assert size(*bad) == 0
    grid = [0, 1, 255, 256, 257, 5000, 100_000, 3_000_000, 2 ** 30 - 1]
    for a, b in zip(grid, grid[1:]):
        assert 0 < size(a, 7) <= size(b, 7) and 0 < size(7, a) <= size(7, b) and size(a, a) <= size(b, b)
    assert size(1000, 1000) % 256 == 0


REFUSED = [
    ((10, F, N, 10, F, N, 0, 0, F, F, F, N), "goi_knn_graph: need 1 <= k <= 16"),
    ((10, F, N, 10, F, N, 17, 0, F, F, F, N), "goi_knn_graph: need 1 <= k <= 16"),
    ((-1, F, N, 10, F, N, 3, 0, F, F, F, N), "goi_knn_graph: bad Pq or Pr"),
    ((10, F, N, -1, F, N, 3, 0, F, F, F, N), "goi_knn_graph: bad Pq or Pr"),
    ((2 ** 30, F, N, 10, F, N, 3, 0, F, F, F, N), "goi_knn_graph: need Pq < 2^30 and Pr < 2^30"),
    ((10, F, N, 10, F, N, 3, 0, N, F, F, N), "goi_knn_graph: a required pointer is NULL"),
    ((10, F, N, 10, F, N, 3, 0, F, N, F, N), "goi_knn_graph: a required pointer is NULL"),
    ((10, N, N, 10, F, N, 3, 0, F, F, F, N), "goi_knn_graph: a required pointer is NULL"),
    ((10, F, N, 10, MIS, N, 3, 1, F, F, F, N), "goi_knn_graph: exclude_self needs queries == refs and Pq == Pr"),
    ((10, F, N, 11, F, N, 3, 1, F, F, F, N), "goi_knn_graph: exclude_self needs queries == refs and Pq == Pr"),
    ((10, F, N, 10, F, N, 3, 1, F, F, N, N), "goi_knn_graph: NULL workspace"),
    ((10, F, N, 10, F, N, 3, 0, F, F, MIS, N), "goi_knn_graph: workspace must be 256-byte aligned"),
]


@pytest.mark.parametrize("args,message", REFUSED)
def test_graph_refusals_before_any_device_call(lib, args, message):
    assert lib.goi_knn_graph(*args) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_majority_refusals_and_empty_calls(lib):
    assert lib.goi_knn_majority(10, 0, F, F, 1.0, 10, F, F, F, N) < 0
    assert lib.goi_raster_last_error().decode() == "goi_knn_majority: need k >= 1"
    assert lib.goi_knn_majority(-1, 3, F, F, 1.0, 10, F, F, F, N) < 0
    assert lib.goi_raster_last_error().decode() == "goi_knn_majority: bad Pq or Pr"
    assert lib.goi_knn_majority(10, 3, F, F, float("nan"), 10, F, F, F, N) < 0
    assert lib.goi_raster_last_error().decode() == "goi_knn_majority: max_dist2 is NaN"
    assert lib.goi_knn_majority(10, 3, F, F, 1.0, 10, F, N, F, N) < 0
    assert lib.goi_raster_last_error().decode() == "goi_knn_majority: a required pointer is NULL"
    assert lib.goi_knn_majority(0, 3, N, N, 1.0, 10, N, N, N, N) == 0  # nothing to do, nothing touched
    assert lib.goi_knn_graph(0, N, N, 10, F, N, 3, 0, N, N, N, N) == 0


def test_python_surface_refuses_cpu_tensors_wrong_dtypes_and_bad_k():
    import torch
    from goi_hyperplane_amd import knn
    import simple_knn._C as drop_in
    assert [n for n in dir(drop_in) if not n.startswith("_")] == ["distCUDA2"]
    pts = torch.zeros(8, 3)
    for call in (lambda: knn.graph(pts, 3), lambda: knn.query(pts, pts, 3), lambda: knn.mean_distance(torch.zeros(8, 3)),
                 lambda: knn.majority_labels(torch.zeros(8, 3, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)),
                 lambda: knn.complete_labels(pts, torch.zeros(8, dtype=torch.int64)), lambda: knn.statistical_outliers(pts, 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="1 <= k <= 16"):
            knn.graph(pts, k)
    with pytest.raises(TypeError):
        knn.graph(pts, 3.0)
