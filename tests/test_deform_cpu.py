"""tests/deform_reference.py checked against mathematics it does not restate, and the inputs of tests/test_gpu_deform.py held to
the condition that makes its bounds tight: no GPU here.

  1. the quaternion iteration converges to the SVD polar factor (U V^T with the determinant fix), on random and on rank-deficient A;
     a zero or rank-1 A leaves q bit for bit;
  2. a rigid image of the rest state is a fixed point, with every node or only three non-collinear nodes constrained;
  3. on the bar the energy never rises (to rounding) and ends below its start;
  4. the unconstrained bipartite chain does not oscillate at the default relax = 0.8 -- and does at relax = 1;
  5. the per-lane SH construction in float64 equals edit.sh_rotation to 1e-12, and D(I) is within 1e-15 of I;
  6. for every GPU case the float32 twin stays within 1e-4 of the float64 run: y of the bounding-box diagonal, q (up to sign)
     absolutely, E of the largest energy the case reaches;
  7. what deform.py refuses before the device matters."""
import inspect

import numpy as np
import pytest
import torch

from tests import deform_cases as cases
from tests import deform_reference as ref
from goi_hyperplane_amd import deform, edit

IDENT = np.array([[1.0, 0, 0, 0]])


def svd_polar(A):
    u, _, vt = np.linalg.svd(A)
    return u @ np.diag([1, 1, np.sign(np.linalg.det(u @ vt))]) @ vt


def random_rotation(rng):
    q = rng.normal(size=4)
    return cases.quat_matrix(q / np.linalg.norm(q)), q / np.linalg.norm(q)


def test_iteration_converges_to_the_svd_polar_factor():
    rng = np.random.default_rng(0)
    for t in range(40):
        A = rng.normal(size=(3, 3))
        if t % 4 == 3:
            A[:, 2] = 0.5 * A[:, 0] - A[:, 1]  # rank 2: the proper polar factor is still unique
        if t % 4 == 2:
            A = -A if np.linalg.det(A) > 0 else A  # det < 0: the proper factor is not the orthogonal one
        s = np.linalg.svd(A)[1]  # (unique iff rank >= 2 and, for det < 0, the two smallest singular values differ)
        if s[1] < 0.1 or (np.linalg.det(A) < 0 and s[1] - s[2] < 0.1):
            continue
        q = ref.polar_steps(A[None], IDENT.copy(), 400)
        assert abs(np.linalg.norm(q) - 1) < 1e-14
        assert np.abs(ref.quat_matrix(q)[0] - svd_polar(A)).max() < 1e-9, t


def test_a_zero_torque_leaves_the_quaternion_bit_for_bit():
    rng = np.random.default_rng(1)
    _, q0 = random_rotation(rng)
    for dtype in (np.float64, np.float32):
        q = q0[None].astype(dtype)
        R = ref.quat_matrix(q)[0].astype(np.float64)
        u = rng.normal(size=3)
        rank1 = np.outer(R @ u, u)  # (y_i - y_j) = R (x_i - x_j) on collinear neighbours: torque r_c x a_c sums to R (u x u) = 0
        for A in (np.zeros((3, 3)), ):
            assert np.array_equal(ref.polar_steps(A[None].astype(dtype), q, 4), q)
        got = ref.polar_steps(rank1[None].astype(dtype), q, 4)
        assert np.abs(got - q).max() < (1e-6 if dtype == np.float32 else 1e-15)


@pytest.mark.parametrize("pins", ["all", "three"])
def test_a_rigid_image_is_a_fixed_point(pins):
    c = cases.bar_case()
    x = c["x"].astype(np.float64)
    R, q = random_rotation(np.random.default_rng(2))
    y = x @ R.T + np.array([0.3, -1.0, 2.0])
    con = np.ones(len(x), np.uint8)
    if pins == "three":
        con[:] = 0
        con[[0, 20, 63]] = 1
    y2, q2 = ref.solve(x, c["idx"], None, con, y, y0=y, q0=np.tile(q, (len(x), 1)), iterations=30)
    assert np.abs(y2 - y).max() < 1e-12
    assert np.abs(q2 - q).max() < 1e-12
    assert ref.energy(x, c["idx"], None, y2, q2) < 1e-24


def test_an_undeformed_graph_keeps_its_bits_in_float32():
    """y = x, q = identity, nodes pinned where they are: every bracket of the position step and the torque are exact zeros"""
    for c in cases.solve_cases():
        x = c["x"]
        con = np.zeros(len(x), np.uint8)
        con[::7] = 1
        y, q = ref.solve(x, c["idx"], c["weight"], con, x, iterations=5, dtype=np.float32)
        assert np.array_equal(y.view(np.uint32), x.view(np.uint32)), c["name"]
        assert np.array_equal(q, np.tile(np.float32([1, 0, 0, 0]), (len(x), 1))), c["name"]


def _energies(c, relax, iterations, dtype=np.float64):
    x = c["x"]
    M = len(x)
    y = x.copy() if c["y0"] is None else c["y0"]
    if c["constrained"] is not None:
        y = np.where(c["constrained"][:, None].astype(bool), c["target"], y)  # the naive edit: only the handle moves
    q = np.tile(IDENT, (M, 1))
    E = [ref.energy(x, c["idx"], c["weight"], y, q)]
    for _ in range(iterations):
        y, q = ref.solve(x, c["idx"], c["weight"], c["constrained"], c["target"], y0=y, q0=q, iterations=1, relax=relax, dtype=dtype)
        E.append(ref.energy(x, c["idx"], c["weight"], y, q))
    return E


def test_energy_never_rises_on_the_bar_and_ends_below_its_start():
    E = _energies(cases.bar_case(), 0.8, 60)
    assert all(b <= a * (1 + 1e-12) for a, b in zip(E, E[1:])), E
    assert E[-1] < 0.05 * E[0]
    E32 = _energies(cases.bar_case(), 0.8, 60, np.float32)
    assert all(b <= a * (1 + 1e-5) for a, b in zip(E32, E32[1:]))


def test_default_relax_matches_the_signature_and_damps_the_bipartite_chain():
    assert inspect.signature(deform.solve).parameters["relax"].default == 0.8
    assert inspect.signature(deform.Deformation.solve).parameters["relax"].default == 0.8
    c = cases.chain_case()
    E = _energies(c, 0.8, 50)
    assert E[-1] < 1e-5 * E[0], E[-1]
    assert all(b <= a * (1 + 1e-12) for a, b in zip(E, E[1:]))
    plain = _energies(c, 1.0, 50)  # the plain Jacobi step keeps the alternating mode for ever
    assert plain[-1] > 1e-3 * plain[0]


def test_lane_sh_construction_equals_the_host_rotation():
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(50):
        R, _q = random_rotation(rng)
        worst = max(worst, np.abs(ref.lane_sh_rotation(R) - edit.sh_rotation(R)).max())
    assert worst < 1e-12, worst
    assert np.abs(ref.lane_sh_rotation(np.eye(3)) - np.eye(16)).max() < 1e-15
    for l, (d, inv) in enumerate(deform.sh_constants(), start=1):
        assert d.shape == (2 * l + 1, 3) and np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15
        assert np.linalg.cond(inv) < 2.0


@pytest.mark.parametrize("c", cases.solve_cases(), ids=lambda c: c["name"])
def test_solve_cases_keep_the_twin_near_float64(c):
    """y within 1e-4 of the bounding-box diagonal, q (up to sign) within 1e-4, E within 1e-4 of the largest energy the case reaches:
    with that, 8 x the twin's error is a bound a wrong kernel cannot meet"""
    x = c["x"]
    diag = float(np.linalg.norm(x.max(0) - x.min(0))) if len(x) > 1 else 1.0
    runs = []
    for it in (1, 2, 25):
        kw = dict(y0=c["y0"], q0=c["q0"], iterations=it)
        y64, q64 = ref.solve(x, c["idx"], c["weight"], c["constrained"], c["target"], dtype=np.float64, **kw)
        y32, q32 = ref.solve(x, c["idx"], c["weight"], c["constrained"], c["target"], dtype=np.float32, **kw)
        assert y32.dtype == np.float32 and q32.dtype == np.float32
        assert np.abs(y32 - y64).max() <= 1e-4 * diag, (c["name"], it)
        assert np.minimum(np.abs(q32 - q64).max(axis=1), np.abs(q32 + q64).max(axis=1)).max() <= 1e-4, (c["name"], it)
        runs.append((ref.energy(x, c["idx"], c["weight"], y64, q64), ref.energy(x, c["idx"], c["weight"], y32, q32)))
    top = max(e64 for e64, _ in runs)
    for e64, e32 in runs:
        assert abs(e32 - e64) <= 1e-4 * top, (c["name"], e64, e32)


@pytest.mark.parametrize("c", cases.apply_cases(), ids=lambda c: c["name"])
def test_apply_cases_keep_the_twin_near_float64(c):
    bind = cases.bind_numpy(c["xyz"], c["nodes"][0], c["kb"], c["mask"])
    a64 = ref.apply(c["xyz"], c["rot"], c["rest"], *bind, c["nodes"], c["sigma"], c["mask"], np.float64, "host")
    a32 = ref.apply(c["xyz"], c["rot"], c["rest"], *bind, c["nodes"], c["sigma"], c["mask"], np.float32, "lane")
    if not len(c["xyz"]):
        return
    diag = float(np.linalg.norm(c["xyz"].max(0) - c["xyz"].min(0))) or 1.0
    assert a32[0].dtype == np.float32
    assert np.abs(a32[0] - a64[0]).max() <= 1e-4 * diag
    assert np.abs(a32[1] - a64[1]).max() <= 1e-4 * np.abs(a64[1]).max()
    if a64[2].size:
        assert np.abs(a32[2] - a64[2]).max() <= 1e-4 * np.abs(a64[2]).max()
    if c["name"].endswith("identity"):
        for got, want in zip(a32[:3], (c["xyz"], c["rot"], c["rest"])):
            assert np.array_equal(got, want)


def test_refusals_before_the_device_matters():
    x = torch.zeros((4, 3))
    idx = torch.zeros((4, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        deform.solve(x, idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        deform.sample_nodes(x, None, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        deform.energy(x, idx, x, torch.zeros((4, 4)))
    for kw, exc in ((dict(relax=0.0), ValueError), (dict(relax=1.5), ValueError), (dict(relax=float("nan")), ValueError),
                    (dict(iterations=-1), ValueError), (dict(iterations=1.5), TypeError), (dict(polar_iters=-1), ValueError),
                    (dict(constrained=torch.zeros(4, dtype=torch.bool)), ValueError), (dict(y0=torch.zeros((3, 3))), ValueError),
                    (dict(q0=torch.zeros((4, 3))), ValueError), (dict(weight=torch.zeros((4, 3))), ValueError),
                    (dict(transposed=(idx,)), TypeError)):
        with pytest.raises(exc):
            deform.solve(x, idx, **kw)
    with pytest.raises(TypeError):
        deform.solve(x.double(), idx)
    with pytest.raises(ValueError):
        deform.solve(x, idx[:3])
    for spacing in (0.0, -1.0, float("inf"), None):
        with pytest.raises((ValueError, TypeError)):
            deform.sample_nodes(x, None, spacing)

    class G:
        _xyz = x
        _rotation = torch.zeros((4, 4))
        _features_rest = torch.zeros((4, 15, 3))
        _semantics_masks = None

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        deform.Deformation(G(), spacing=0.5)
    for kw in (dict(spacing=0.5, kb=9), dict(spacing=0.5, kb=0), dict(spacing=0.5, k=0), dict(spacing=-1.0)):
        with pytest.raises(ValueError):
            deform.Deformation(G(), **kw)
    masked = G()
    masked._semantics_masks = torch.zeros(4)
    with pytest.raises(ValueError, match="semantic mask"):
        deform.Deformation(masked, spacing=0.5)
