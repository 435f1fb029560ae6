"""The adversarial DBSCAN inputs (tests/dbscan_cases.py) deserve their names, shown without a GPU from the two restatements
alone: the exact fp32 fma, the threshold classes and the discriminating power of every variant (the counts are printed:
run with -s), agreement of the k-d-tree restatement with the brute force, isolation of the molecules and the clustering
that follows from the bond classes, the key-layout coverage, the chain's cluster count, the axis-limit step and the absence
of subnormal squares on the scaled inputs of the GPU tests.

Mutation check: test_alternative_forms_change_the_labels puts each d2_alt kind in the place of the kernel's form in
dbscan_brute and requires the comparison with dbscan_reference to FAIL on the threshold, key-layout, stack and chain
cases, by >= 100 core / noise decisions on every threshold variant at min_samples 2 and 3."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.spatial import cKDTree

from tests import dbscan_cases as dc
from tests.dbscan_reference import (ALT_KINDS, BRUTE_MAX_N, _fma32, _fma32_double_rounding, brute_neighbours, d2_form,
                                    dbscan_reference, is_neighbour, labels_from_neighbours)

F32, F64 = np.float32, np.float64
VARIANTS = list(dc.THRESHOLD_VARIANTS)
BRUTE_CASES = [n for n in dc.CASES if n != "chain" and not (n.startswith("cloud") and dc.CLOUDS[n][0] > BRUTE_MAX_N)]
SCALED_CASES = dc.MOLECULE_CASES + dc.STACK_CASES


def _fraction_fma32(a, b, c):
    """fl32(a * b + c) by exact rational arithmetic: the fp32 neighbours of the exact value, the nearer one, ties to even."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = F32(float(exact))  # (a float64 rounding first: only used to find the bracket)
    cands = sorted({float(near), float(np.nextafter(near, F32(-np.inf))), float(np.nextafter(near, F32(np.inf)))})
    best = min(cands, key=lambda v: (abs(Fraction(v) - exact), int(F32(v).view(np.uint32)) & 1))
    return F32(best)


def test_fma32_equals_exact_arithmetic_on_random_triples():
    rng = np.random.default_rng(5)
    n = 20000
    a = (rng.normal(size=n) * np.exp2(rng.integers(-12, 12, n))).astype(F32)
    b = (rng.normal(size=n) * np.exp2(rng.integers(-12, 12, n))).astype(F32)
    c = (rng.normal(size=n) * np.exp2(rng.integers(-24, 24, n))).astype(F32)
    c[: n // 4] = (-a[: n // 4].astype(F64) * b[: n // 4].astype(F64)).astype(F32)  # cancellation
    c[n // 4: n // 2] = (a[n // 4: n // 2] * a[n // 4: n // 2])  # the kernel's use: fma(dy, dy, dx * dx)
    b[n // 4: n // 2] = a[n // 4: n // 2] * F32(0.37)
    a[n // 4: n // 2] = b[n // 4: n // 2]
    got = _fma32(a, b, c)
    want = np.array([_fraction_fma32(x, y, z) for x, y, z in zip(a, b, c)], F32)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_fma32_breaks_midpoint_ties_by_the_error_term():
    """The float64 sum lies exactly half-way between two fp32 values and the part that float64 dropped decides.  With
    up = 1 + 2^-23 and dn = 1 - 2^-23, up * (2^-24 dn) = 2^-24 - 2^-70: added to an fp32 number near 1 it gives a midpoint
    less (or, negated, plus) 2^-70, which float64 drops.  Rounding the float64 sum again sends the midpoint to the even
    neighbour, which is the wrong one in the first three cases."""
    one, u = F32(1.0), F32(2.0 ** -23)
    up, dn, q = one + u, one - u, F32(2.0 ** -24)
    cases = [  # a, b, c                exact sum                                  fl32
        (up, q * dn, up),             # 1 + 2^-23 + 2^-24 - 2^-70: below the midpoint: 1 + 2^-23 (odd)
        (up, -q * dn, up),            # 1 + 2^-24 + 2^-70:         above the midpoint: 1 + 2^-23 (odd)
        (-up, q * dn, -up),           # the mirror image of the first:                 -(1 + 2^-23)
        (up, q * dn, one),            # 1 + 2^-24 - 2^-70:         below the midpoint: 1 (even: both emulations agree)
        (up, -q * dn, one + u + u),   # 1 + 2^-23 + 2^-24 + 2^-70: above the midpoint: 1 + 2^-22 (even)
    ]
    a, b, c = (np.array(v, F32) for v in zip(*cases))
    s64 = a.astype(F64) * b.astype(F64) + c.astype(F64)
    for s in s64:  # every float64 sum is the midpoint of two adjacent fp32 values, not one of them
        r = F32(s)
        assert F64(r) != s
        assert any(F64(r) + F64(np.nextafter(r, F32(t))) == 2 * s for t in (-np.inf, np.inf))
    want = np.array([_fraction_fma32(x, y, z) for x, y, z in cases], F32)
    np.testing.assert_array_equal(want, np.array([up, up, -up, one, one + u + u], F32))
    np.testing.assert_array_equal(_fma32(a, b, c), want)
    old = _fma32_double_rounding(a, b, c)
    np.testing.assert_array_equal(old != want, [True, True, True, False, False])


# ---------------------------------------------------------------------------------------------------------------- helpers
@functools.lru_cache(maxsize=None)
def reference(name):
    pts, eps, ms = dc.get(name)
    return dbscan_reference(pts, eps, ms)


def _point_set(name):
    """Cases that differ only in min_samples share their points: one neighbour matrix serves them all."""
    return name.rsplit("_ms", 1)[0] if "_ms" in name and not name.startswith(("cloud", "stacks")) else name


@functools.lru_cache(maxsize=None)
def _neighbours(point_set, kind):
    name = next(n for n in dc.CASES if _point_set(n) == point_set)
    pts, eps, _ = dc.get(name)
    return brute_neighbours(pts, eps, kind)


def brute(name, kind="kernel"):
    return labels_from_neighbours(_neighbours(_point_set(name), kind), dc.get(name)[2])


def bond_decisions(name, kind="kernel"):
    pts, eps, _ = case = dc.get(name)
    b = case.meta["bonds"]
    return is_neighbour(pts[b[:, 0]], pts[b[:, 1]], eps, kind)


def decisions_changed(a, b):
    """Points whose core flag or noise status differs between two (labels, core) results."""
    return int(((a[1] != b[1]) | ((a[0] < 0) != (b[0] < 0))).sum())


def labels_from_bonds(case):
    """The clustering that follows from the bond classes alone (classes <= 0 hold), molecules being isolated."""
    n = len(case[0])
    b = case.meta["bonds"][case.meta["bond_class"] <= 0]
    i = np.concatenate([np.arange(n), b[:, 0], b[:, 1]])
    j = np.concatenate([np.arange(n), b[:, 1], b[:, 0]])
    return labels_from_neighbours(coo_matrix((np.ones(len(i), bool), (i, j)), shape=(n, n)).tocsr(), case[2])


# ------------------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(dc.CASES))
def test_cases_are_well_formed(name):
    pts, eps, ms = case = dc.get(name)
    assert pts.dtype == F32 and pts.ndim == 2 and pts.shape[1] == 3 and 0 < len(pts) <= 30000
    assert np.isfinite(pts).all() and isinstance(eps, float) and isinstance(ms, int)
    again = dc.CASES[name](dc.SEED)
    np.testing.assert_array_equal(again[0], pts)  # a function of the seed
    src = case.meta.get("source_index")
    if src is not None and len(src) > 8:
        assert (np.diff(src) < 0).any() and (np.diff(src) > 0).any()  # arrives permuted


@pytest.mark.parametrize("variant", VARIANTS)
def test_threshold_classes_and_discriminating_power(variant):
    name = f"threshold_{variant}_ms2"
    pts, eps, _ = case = dc.get(name)
    b, cls, kind = case.meta["bonds"], case.meta["bond_class"], case.meta["bond_kind"]
    d2 = d2_form(pts[b[:, 0]], pts[b[:, 1]])
    vals = dc.class_values(eps)
    counts = [int((d2 == v).sum()) for v in vals]
    np.testing.assert_array_equal(d2, vals[cls + 1])  # the bookkeeping is the arithmetic
    kern = bond_decisions(name)
    np.testing.assert_array_equal(kern, cls <= 0)
    flips = {k: int((bond_decisions(name, k) != kern).sum()) for k in ALT_KINDS}
    cells = dc.cell_indices(pts, eps)
    span = np.abs(cells[b[:, 0]] - cells[b[:, 1]]).max(axis=1)
    two_cells = int(((span == 2) & (kind == 1) & kern).sum())
    print(f"\n{name}: n={len(pts)} bonds={len(b)} pred/tie/succ={counts} decided differently {flips}; "
          f"holding axis bonds two cells apart: {two_cells}; per direction kind {np.bincount(kind).tolist()}")
    assert min(counts) >= 200
    assert min(flips.values()) >= 50
    assert two_cells >= 100 and span.max() == 2
    assert np.bincount(kind, minlength=3).min() >= 200  # every direction kind is represented as well as a class


@pytest.mark.parametrize("ms", [2, 3])
@pytest.mark.parametrize("variant", VARIANTS)
def test_alternative_forms_change_the_labels(variant, ms):
    """The mutation check on the threshold sets: the brute force with another form in place of the kernel's differs from
    the restatement in >= 100 core / noise decisions."""
    name = f"threshold_{variant}_ms{ms}"
    ref = reference(name)
    assert decisions_changed(brute(name), ref) == 0
    changed = {k: decisions_changed(brute(name, k), ref) for k in ALT_KINDS}
    print(f"\n{name}: core / noise decisions an alternative form gets wrong {changed}")
    assert min(changed.values()) >= 100


@pytest.mark.parametrize("name", ["key_layout_ms2", "key_layout_ms3", "stacks_ms2", "stacks_ms64", "stacks_ms65",
                                  "stacks_ms257", "chain_short"])
def test_alternative_forms_change_the_labels_elsewhere(name):
    """The same mutation check on the cases with fewer threshold bonds: every alternative form fails the comparison."""
    ref = reference(name)
    changed = {}
    for k in ALT_KINDS:
        got = brute(name, k)
        changed[k] = (decisions_changed(got, ref), int((got[0] != ref[0]).sum()))
    print(f"\n{name}: (core / noise decisions, labels) an alternative form gets wrong {changed}")
    assert all(labels > 0 for _, labels in changed.values())


@pytest.mark.parametrize("name", BRUTE_CASES)
def test_restatement_equals_brute_force(name):
    want, want_core = brute(name)
    got, got_core = reference(name)
    np.testing.assert_array_equal(got_core, want_core)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", dc.MOLECULE_CASES + dc.STACK_CASES)
def test_molecules_are_isolated(name):
    pts, eps, _ = case = dc.get(name)
    mol = case.meta["molecule"]
    pairs = cKDTree(pts.astype(F64)).query_pairs(2.0 * eps * (1 + 1e-6), output_type="ndarray")
    assert (mol[pairs[:, 0]] == mol[pairs[:, 1]]).all()
    assert len(pairs) >= len(case.meta["bonds"]) - 2


@pytest.mark.parametrize("name", dc.MOLECULE_CASES + ["chain", "chain_short"])
def test_clustering_follows_from_the_bond_classes(name):
    case = dc.get(name)
    want, want_core = labels_from_bonds(case)
    got, got_core = reference(name)
    cls = case.meta["bond_class"]
    print(f"\n{name}: n={len(case[0])} min_samples={case[2]} clusters={got.max() + 1} noise={int((got < 0).sum())} "
          f"bonds holding / not {int((cls <= 0).sum())} / {int((cls > 0).sum())}")
    np.testing.assert_array_equal(got_core, want_core)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(bond_decisions(name), cls <= 0)


@pytest.mark.parametrize("ms", dc.STACK_MS)
def test_stacks_straddle_min_samples(ms):
    name = f"stacks_ms{ms}"
    pts, eps, _ = case = dc.get(name)
    m = case.meta
    _, core = reference(name)
    cells = dc.cell_indices(pts, eps)
    one_cell = np.array([(cells[g] == cells[g[0]]).all() for g in m["groups"]])
    ks = sorted(set(m["stack_k"].tolist()))
    assert ks == [k for k in (ms - 1, ms, ms + 1) if k >= 1]
    for k in ks:
        sel = m["stack_k"] == k
        holds = m["bond_class"][sel] <= 0
        print(f"\n{name}: k={k} stacks={int(sel.sum())} in one cell={int(one_cell[sel].sum())} "
              f"satellite classes {np.bincount(m['bond_class'][sel] + 1, minlength=3).tolist()}")
        assert sel.sum() >= 8 and one_cell[sel].sum() >= 6 and 0 < holds.sum() < sel.sum()
        # the contact has its k stack mates (itself included) and, when the bond holds, the satellite
        np.testing.assert_array_equal(core[m["contact"][sel]], (k + holds) >= ms)
    for g in m["groups"]:
        assert (np.abs(pts[g].astype(F64) - pts[g[0]].astype(F64)) <= 0.0101 * eps).all()


def test_key_layout_coverage():
    pts, eps, _ = case = dc.get("key_layout_ms2")
    cells = dc.cell_indices(pts, eps)
    b = case.meta["bonds"][case.meta["bond_class"] <= 0]
    ca, cb = cells[b[:, 0]], cells[b[:, 1]]
    word = int((ca[:, 1] >> 11 != cb[:, 1] >> 11).sum())
    dz = int((ca[:, 2] != cb[:, 2]).sum())
    beyond = [int((cells[:, a] > 2 ** 20).sum()) for a in range(3)]
    print(f"\nkey_layout: n={len(pts)} holding bonds={len(b)}; cy on either side of a multiple of 2^11: {word}; cz different: "
          f"{dz}; points beyond cell 2^20 per axis {beyond}; largest cell {cells.max(axis=0).tolist()}")
    assert word >= 64 and dz >= 64
    assert min(beyond) >= 50 and cells.max() < 2 ** 21 - 1
    # only one axis is large at a time (the arms), and cells 0 and 1 of every axis are occupied
    assert ((cells > 2 ** 20).sum(axis=1) <= 1).all()
    for a in range(3):
        assert (cells[:, a] == 0).any() and (cells[:, a] == 1).any()
    assert (cells == 0).all(axis=1).any() and (cells == 1).all(axis=1).any()


@pytest.mark.parametrize("name", ["chain", "chain_short"])
def test_chain_is_one_filament_with_b_breaks(name):
    pts, eps, ms = case = dc.get(name)
    assert ms == 2 and (name != "chain" or len(pts) >= 20000)
    along = case.meta["source_index"]
    cls = case.meta["bond_class"]
    breaks = int((cls > 0).sum())
    labels, core = reference(name)
    assert breaks >= 30 and labels.max() + 1 == breaks + 1 and (labels >= 0).all() and core.all()
    order = np.argsort(along)
    step = np.linalg.norm(np.diff(pts[order].astype(F64), axis=0), axis=1) / eps
    plain = cls == -2
    assert step[plain].min() >= 0.6 and step[plain].max() <= 0.9 and abs(step[~plain] - 1).max() < 1e-3
    near = cKDTree(pts.astype(F64)).query_pairs(2.0 * eps, output_type="ndarray")
    # never within 2 eps of itself: such pairs are at most 4 links apart (round a corner the chord is >= path / sqrt(2), so
    # a chord <= 2 eps spans a path <= 2.83 eps, fewer than 5 links of >= 0.6 eps; parallel rows are 3 eps apart)
    assert np.abs(along[near[:, 0]] - along[near[:, 1]]).max() <= 4
    # with and against the key order (z, then y, then x): the cell key rises along some links and falls along others
    cells = dc.cell_indices(pts[order], eps)
    key = cells[:, 0] + (cells[:, 1] << 21) + (cells[:, 2] << 42)
    rising, falling = int((np.diff(key) > 0).sum()), int((np.diff(key) < 0).sum())
    own_cell = len(np.unique(key)) / len(key)
    print(f"\n{name}: n={len(pts)} breaks={breaks} clusters={labels.max() + 1} links with / against the key order "
          f"{rising} / {falling}; cells per point {own_cell:.2f}")
    assert min(rising, falling) >= len(pts) // 4 and own_cell > 0.9


def test_axis_limit_inputs_are_one_step_apart():
    ok, over = dc.get("axis_limit"), dc.axis_limit(dc.SEED, over=True)
    h = dc.cell_side(ok[1])
    x_ok, x_over = ok[0][:, 0].max(), over[0][:, 0].max()
    assert np.nextafter(x_ok, F32(np.inf)) == x_over and ok[0][:, 0].min() == 0 == over[0][:, 0].min()
    assert F64(x_ok) / h < 2 ** 21 - 1 <= F64(x_over) / h
    cells = dc.cell_indices(ok[0], ok[1])
    assert cells[:, 0].max() == 2 ** 21 - 2
    labels, core = reference("axis_limit")
    assert labels.max() + 1 == 2 and core.all()
    print(f"\naxis_limit: X = {x_ok!r} (cell {cells[:, 0].max()}), refused from {x_over!r}")


def test_eps_limit_inputs_scale_exactly():
    base = dc.eps_limit(dc.SEED, k=0)
    want = dbscan_reference(*base)
    assert base[1] == 0.5 and want[0].max() + 1 == 2 and (want[0] < 0).sum() == 1
    for name, eps in (("eps_limit_lo", 2.0 ** -40), ("eps_limit_hi", 2.0 ** 40)):
        pts, e, _ = dc.get(name)
        assert e == eps
        np.testing.assert_array_equal(pts, np.ldexp(base[0], int(np.log2(eps / 0.5))))
        got = reference(name)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("name", SCALED_CASES)
def test_no_subnormal_square_on_the_scaled_inputs(name):
    """The GPU tests scale these inputs by 2^-30 and 2^30.  Every pair the kernel can look at (same +-2 window: less than
    3 eps apart) has squares of its coordinate differences that are 0 or normal fp32 numbers after the scaling, and nothing
    overflows, so each operation of the form scales exactly and the labels must not change."""
    pts, eps, _ = dc.get(name)
    pairs = cKDTree(pts.astype(F64)).query_pairs(3.0 * eps, output_type="ndarray")
    tiny, huge = np.finfo(F32).tiny, np.finfo(F32).max
    for k in (-30, 30):
        if not 2.0 ** -40 <= eps * 2.0 ** k <= 2.0 ** 40:  # (the eps-limit inputs already sit at an end of the range)
            continue
        x = np.ldexp(pts, k).astype(F32)
        np.testing.assert_array_equal(np.ldexp(x.astype(F64), -k), pts.astype(F64))  # the scaling itself is exact
        d = x[pairs[:, 0]] - x[pairs[:, 1]]
        sq = d * d
        assert ((sq == 0) | (sq >= tiny)).all() and (d2_form(x[pairs[:, 0]], x[pairs[:, 1]]) < huge).all()
        span = (x.max(axis=0) - x.min(axis=0)).astype(F64)
        assert 3 * (span ** 2).sum() < huge
