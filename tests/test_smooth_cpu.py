"""goi_hyperplane_amd.smooth without a GPU: the numpy restatement the kernels are held to
(tests/smooth_reference.py) against float64 autograd of the literal formula, its float32 order against its float64 truth within
the derived bounds, the transpose against the definition, diffusion's range, copies and convergence, the descent property that
pins the gradient's sign and scale, what the shared case list (tests/smooth_cases.py) covers, and every refusal of the Python
surface."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import smooth_cases as sc
from tests import smooth_reference as ref


@pytest.mark.parametrize("name", sc.names())
def test_float64_restatement_is_the_literal_formula_and_its_autograd_gradient(name):
    L, g, ne = sc.reference(name, np.float64)
    want_L, want_g = sc.autograd64(name)
    assert ne == ref.n_edges(sc.case(name)["idx"], sc.case(name)["rows"])
    assert abs(L - want_L) <= 1e-12 * abs(want_L)
    assert np.abs(g - want_g).max() <= 1e-12 * np.abs(want_g).max()


@pytest.mark.parametrize("name", sc.SMALL)
def test_transpose_is_the_double_loop(name):
    idx = sc.case(name)["idx"]
    in_ptr, in_edge = sc.transposed(name)
    want_ptr, want_edge = ref.transpose_double_loop(idx)
    assert in_ptr.dtype == in_edge.dtype == np.int32
    assert np.array_equal(in_ptr, want_ptr) and np.array_equal(in_edge, want_edge)
    assert in_ptr[-1] == ref.edge_mask(idx).sum() and np.all(in_edge[in_ptr[-1]:] == -1)


@pytest.mark.parametrize("name", sc.names())
def test_transpose_lists_every_edge_once_under_its_target_in_edge_order(name):
    idx = sc.case(name)["idx"]
    P, k = idx.shape
    in_ptr, in_edge = sc.transposed(name)
    E = int(in_ptr[-1])
    assert E == ref.edge_mask(idx).sum() and np.all(in_edge[E:] == -1)
    assert np.array_equal(np.sort(in_edge[:E]), np.flatnonzero(ref.edge_mask(idx).reshape(-1)))
    target = idx.reshape(-1)[in_edge[:E]]
    assert np.array_equal(target, np.repeat(np.arange(P), np.diff(in_ptr)))
    same = target[1:] == target[:-1]
    assert np.all(in_edge[1:E][same] > in_edge[:E - 1][same])


@pytest.mark.parametrize("name", sc.names())
def test_float32_order_is_within_the_derived_bounds_of_float64(name):
    """These bounds are derived (smooth_reference.loss_chain, grad_bound), not tuned: a failure means the documented order and the
    restatement differ."""
    c = sc.case(name)
    L32, g32, ne32 = sc.reference(name, np.float32)
    L64, g64, ne64 = sc.reference(name, np.float64)
    assert L32.dtype == np.float32 and g32.dtype == np.float32 and ne32 == ne64
    S, k = c["f"].shape[1], c["idx"].shape[1]
    assert abs(float(L32) - float(L64)) <= ref.gamma(ref.loss_chain(S, k)) * float(L64)
    assert np.all(np.abs(g32.astype(np.float64) - g64) <= sc.gradient_bound(name))
    if ne64 == 0:
        assert float(L32) == 0 and not g32.any()


def test_the_case_list_covers_what_it_is_there_for():
    cs = sc.cases()
    assert max(c["f"].shape[0] for c in cs) <= 20000
    assert {c["f"].shape[0] for c in cs} >= {1, 2, 63, 64, 65, 257, 1000}
    assert {c["f"].shape[1] for c in cs} >= {1, 3, 16, 17, 32}
    assert {c["idx"].shape[1] for c in cs} >= {1, 3, 8, 16}
    star = sc.case("star_P5000_S16_k1")
    deg = np.diff(sc.transposed("star_P5000_S16_k1")[0])
    assert deg.max() == deg[0] == 4999 and deg[1:].max() == 0  # every other row points at row 0
    assert (star["idx"][1:] == 0).all() and star["idx"][0, 0] == -1
    hubs = np.diff(sc.transposed("two_hubs_P1000_S17_k16")[0])
    assert hubs[0] >= 1000 and hubs[1] >= 1000
    assert any(ref.n_edges(c["idx"], c["rows"]) == 0 for c in cs)
    assert any(c["rows"] is not None and not c["rows"].any() and ref.edge_mask(c["idx"]).any() for c in cs)
    assert any((~ref.edge_mask(c["idx"]).any(axis=1)).any() for c in cs)                       # a row with no edge
    assert any((np.diff(sc.transposed(c["name"])[0]) == 0).any() and c["f"].shape[0] > 1 for c in cs)  # an in-degree-0 row
    assert any((c["idx"] >= c["f"].shape[0]).any() for c in cs)                                # an id >= P
    assert any((c["idx"] == np.arange(c["f"].shape[0])[:, None]).any() for c in cs)            # a self edge
    dup = sc.case("duplicates_P63_S3_k8")["idx"]
    assert all(len(set(r)) < len(r) for r in dup.tolist())
    assert any(c["weight"] is not None and (c["weight"] == 0).any() for c in cs)
    assert any(c["weight"] is None for c in cs) and any(c["rows"] is None for c in cs)
    assert any((c["idx"] == -1).all(axis=1).any() and c["f"].shape[0] > 1 for c in cs)          # a whole -1 row
    # an in-list longer than one batch of 16, and one that ends inside a batch
    assert any(((d := np.diff(sc.transposed(c["name"])[0])) > 16).any() and (d % 16 != 0).any() for c in cs)


def test_a_self_edge_counts_and_adds_zero():
    f = np.array([[1.0, 2.0], [4.0, -1.0]], np.float32)
    idx = np.array([[0, 1], [1, 1]], np.int32)
    L, g, ne = ref.loss_and_grad(f, idx, dtype=np.float64)
    assert ne == 4 and L == (9 + 9) / 4
    assert np.array_equal(g, (2 / 4) * np.array([[-3.0, 3.0], [3.0, -3.0]]))


# ---- diffusion ------------------------------------------------------------------------------------------------------------------
DIFFUSE = ["knn_P63_S16_k8", "knn_P257_S3_k8", "tails_P257_S17_k8", "self_edges_P64_S32_k3", "random_P1000_S1_k16",
           "ids_out_of_range_P65_S16_k3"]


@pytest.mark.parametrize("lam", [1.0, 0.5])
@pytest.mark.parametrize("name", DIFFUSE)
def test_diffusion_stays_inside_what_it_averages_and_copies_the_rest(name, lam):
    """out = f + lam (m - f) with 0 <= lam <= 1 and m a weighted mean with non-negative weights: exactly, every element lies between
    the minimum and the maximum of the row's own value and its neighbours'.  In float32 the numerator and W go through at most k
    additions and one product each (gamma(k + 1) relative to W max|f|, gamma(k) for W), the quotient, the difference, the product
    with lam and the last sum one rounding each on values of at most 2 max|f|: gamma(2 k + 8) * 2 max|f| covers all of it."""
    c = sc.case(name)
    f, idx, w = c["f"], c["idx"], c["weight"]
    P, k = idx.shape
    fixed = np.random.default_rng(3).random(P) < 0.3
    out = ref.diffuse(f, idx, w, fixed, lam, 1, np.float32)
    assert out.dtype == np.float32 and out.shape == f.shape
    edge = ref.edge_mask(idx)
    nb = f[np.where(edge, idx, np.arange(P)[:, None])]  # [P,k,S], the own row where a slot is no edge
    lo, hi = np.minimum(nb.min(axis=1), f), np.maximum(nb.max(axis=1), f)
    tol = ref.gamma(2 * k + 8) * 2 * np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64)
    assert np.all(out >= lo - tol) and np.all(out <= hi + tol)
    wsum = edge.sum(axis=1) if w is None else np.where(edge, w, 0).sum(axis=1)
    copied = fixed | ~edge.any(axis=1) | (wsum == 0)
    assert copied.any() and (~copied).any()
    assert np.array_equal(out[copied].view(np.uint32), f[copied].view(np.uint32))
    assert np.any(out[~copied] != f[~copied])
    # five steps are five single steps
    five = ref.diffuse(f, idx, w, fixed, lam, 5, np.float32)
    step = f
    for _ in range(5):
        step = ref.diffuse(step, idx, w, fixed, lam, 1, np.float32)
    assert np.array_equal(five, step)


def test_two_clusters_converge_to_their_fixed_values():
    """Two clusters without an edge between them, the fixed rows of each sharing one value: the fixed point of the iteration is
    that value on every row that reaches a fixed row along out-edges (here: all).  lam = 1/2 (the lazy iteration) cannot cycle."""
    rng = np.random.default_rng(0)
    n, k, S = 40, 3, 3
    idx = np.empty((2 * n, k), np.int32)
    for c in range(2):
        idx[c * n:(c + 1) * n] = rng.integers(0, n, (n, k)) + c * n
        idx[c * n + 1:(c + 1) * n, 0] = np.arange(c * n, (c + 1) * n - 1)  # row i -> i - 1: a path to the cluster's first row
    fixed = np.zeros(2 * n, bool)
    fixed[[0, 7, 19, n, n + 3]] = True
    values = np.array([[1.0, -2.0, 0.5], [-4.0, 3.0, 8.0]])
    f = rng.standard_normal((2 * n, S)).astype(np.float32)
    for c in range(2):
        f[c * n:(c + 1) * n][fixed[c * n:(c + 1) * n]] = values[c]
    assert not np.any((idx[:n] >= n) | (idx[n:] < n))  # no edge between the clusters
    reach = fixed.copy()  # every row reaches a fixed row along out-edges
    for _ in range(2 * n):
        reach |= reach[idx].any(axis=1)
    assert reach.all()
    want = np.repeat(values, n, axis=0)
    cur, steps = f.astype(np.float64), 0
    while np.abs(cur - want).max() > 1e-9 and steps < 20000:
        cur = ref.diffuse(cur, idx, None, fixed, 0.5, 50, np.float64)
        steps += 50
    assert np.abs(cur - want).max() <= 1e-9, steps
    before = np.abs(f.astype(np.float64) - want).max()
    assert before > 1 and np.array_equal(cur[fixed], want[fixed])


# ---- the descent property: sign and scale of the gradient -------------------------------------------------------------------------
DESCENT = ["knn_P257_S3_k8", "knn_P1000_S16_k16", "two_hubs_P1000_S17_k16", "tails_P257_S17_k8", "star_weighted_P5000_S3_k1"]


@pytest.mark.parametrize("name", DESCENT)
def test_ten_gradient_steps_never_increase_the_loss(name):
    """L is a quadratic form whose Hessian is (2 / N_E) times twice a weighted graph Laplacian: its largest eigenvalue is at most
    4 d_max / N_E, so a step of N_E / (4 d_max) along -gradient cannot increase L.  A gradient of the wrong sign increases it and
    one that is too large by a factor above 2 overshoots."""
    c = sc.case(name)
    idx, w, rows = c["idx"], c["weight"], c["rows"]
    ne, d_max = ref.n_edges(idx, rows), ref.weight_degree(idx, w, rows)
    assert ne > 0 and d_max > 0
    T = sc.transposed(name)
    f = c["f"].astype(np.float64)
    last, first = None, None
    for _ in range(11):
        L, g, _ = ref.loss_and_grad(f, idx, w, rows, np.float64, T)
        assert last is None or L <= last
        first = L if first is None else first
        last = L
        f = f - (ne / (4 * d_max)) * g
    assert last < first
    # the same steps with the sign flipped go up
    L_up, _, _ = ref.loss_and_grad(c["f"].astype(np.float64) + (ne / (4 * d_max)) * sc.reference(name, np.float64)[1], idx, w, rows,
                                   np.float64, T)
    assert L_up > first


# ---- the Python surface -------------------------------------------------------------------------------------------------------------
def test_module_is_exported():
    import goi_hyperplane_amd
    from goi_hyperplane_amd import smooth
    assert goi_hyperplane_amd.smooth is smooth and "smooth" in goi_hyperplane_amd.__all__
    for name in ("transpose", "loss", "loss_terms", "gaussian_weights", "diffuse", "complete_features"):
        assert callable(getattr(smooth, name))


def test_python_refusals():
    from goi_hyperplane_amd import smooth
    f = torch.zeros(8, 4)
    idx = torch.zeros(8, 3, dtype=torch.int32)
    w = torch.ones(8, 3)
    rows = torch.ones(8, dtype=torch.bool)
    T = (torch.zeros(9, dtype=torch.int32), torch.zeros(24, dtype=torch.int32))
    # CPU tensors: there is no CPU fallback
    for call in (lambda: smooth.transpose(idx), lambda: smooth.loss(f, idx), lambda: smooth.loss_terms(f, idx, w, rows, T),
                 lambda: smooth.gaussian_weights(w, 1.0), lambda: smooth.diffuse(f, idx, w, rows),
                 lambda: smooth.complete_features(torch.zeros(8, 3), f, rows)):
        with pytest.raises(RuntimeError, match="there is no CPU fallback"):
            call()
    # dtypes and non-tensors
    for call in (lambda: smooth.transpose(idx.long()), lambda: smooth.transpose(idx.numpy()), lambda: smooth.loss(f.double(), idx),
                 lambda: smooth.loss(f, idx.long()), lambda: smooth.loss(f, idx, w.double()), lambda: smooth.loss(f, idx, None, rows.float()),
                 lambda: smooth.loss(f, idx, transposed=(T[0].long(), T[1])), lambda: smooth.loss(f, idx, transposed=T[0]),
                 lambda: smooth.loss(None, idx), lambda: smooth.gaussian_weights(w.double(), 1.0), lambda: smooth.gaussian_weights(1.0, 1.0),
                 lambda: smooth.diffuse(f.half(), idx), lambda: smooth.diffuse(f, idx, fixed=rows.int()),
                 lambda: smooth.diffuse(f, idx, iterations=2.0), lambda: smooth.diffuse(f, idx, iterations=True),
                 lambda: smooth.complete_features(torch.zeros(8, 3), f, None), lambda: smooth.complete_features(torch.zeros(8, 3), f, rows.float())):
        with pytest.raises(TypeError):
            call()
    # shapes and ranges
    for call in (lambda: smooth.transpose(idx[0]), lambda: smooth.transpose(torch.zeros(8, 0, dtype=torch.int32)),
                 lambda: smooth.transpose(torch.empty((2 ** 30, 1), dtype=torch.int32, device="meta")),
                 lambda: smooth.transpose(torch.empty((2 ** 26, 16), dtype=torch.int32, device="meta")),
                 lambda: smooth.loss(torch.zeros(8, 33), idx), lambda: smooth.loss(torch.zeros(8, 0), idx), lambda: smooth.loss(f[0], idx),
                 lambda: smooth.loss(f, idx[:7]), lambda: smooth.loss(f, idx, w[:, :2]), lambda: smooth.loss(f, idx, None, rows[:7]),
                 lambda: smooth.loss(f, idx, transposed=(T[0][:8], T[1])), lambda: smooth.loss(f, idx, transposed=(T[0], T[1][:23])),
                 lambda: smooth.gaussian_weights(w[0], 1.0), lambda: smooth.gaussian_weights(w, 0.0), lambda: smooth.gaussian_weights(w, -1.0),
                 lambda: smooth.gaussian_weights(w, float("nan")), lambda: smooth.gaussian_weights(w, float("inf")),
                 lambda: smooth.diffuse(f, idx, iterations=-1), lambda: smooth.diffuse(f, idx, lam=float("nan")),
                 lambda: smooth.diffuse(f, idx, fixed=rows[:7]), lambda: smooth.diffuse(torch.zeros(8, 40), idx),
                 lambda: smooth.complete_features(torch.zeros(7, 3), f, rows), lambda: smooth.complete_features(torch.zeros(8, 3), f, rows[:7])):
        with pytest.raises(ValueError):
            call()
