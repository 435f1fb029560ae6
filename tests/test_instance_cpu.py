"""The numpy restatement of goi_hyperplane_amd.instance (tests/instance_reference.py) against exact arithmetic on every case of
tests/instance_cases.py, and the module's argument checks.  No GPU.

The exact side is fractions.Fraction throughout (sums of w, w x, w x x^T and w f over the raw positions: math.fsum is not used,
because the covariance needs exact products of three numbers); integers are compared exactly, every float within the bound
derived in instance_reference.py's docstring -- derived, not measured.  The restatement's worst ratio to its bound is printed
(run with -s)."""
from __future__ import annotations

import struct

import numpy as np
import pytest
import torch

from tests import instance_cases as ic
from tests import instance_reference as ref


def test_the_case_list_covers_every_bullet():
    covered = set().union(*(c["tags"] for c in ic.cases()))
    assert covered == set(ic.TAGS), sorted(set(ic.TAGS) - covered)
    sizes = set()
    for c in ic.cases():
        ptr, _, _ = ic.reference(c["name"])
        sizes |= set(np.diff(ptr).tolist())
        assert c["label"].shape[0] <= 20000
    assert {0, 1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 5000} <= sizes
    assert {c["features"].shape[1] for c in ic.cases() if c["features"] is not None} >= {1, 3, 16, 17, 32}
    assert {c["label"].shape[0] > 256 for c in ic.cases()} == {True, False}  # both sides of the slot path's threshold
    hits = ic.case("all_sizes_S16")["hit"]
    assert hits.dtype == np.uint8 and set(hits.tolist()) == set(range(256))
    rows = ic.reference("all_sizes_S16")[1]
    inside = rows[rows >= 0]
    assert not np.array_equal(inside, np.sort(inside)), "member must be a real permutation"


@pytest.mark.parametrize("name", ic.names())
def test_members_are_the_rows_of_each_label_in_ascending_order(name):
    c = ic.case(name)
    ptr, rows, _ = ic.reference(name)
    label, K, P = c["label"], c["K"], c["label"].shape[0]
    assert ptr.dtype == rows.dtype == np.int32 and ptr.shape == (K + 1,) and rows.shape == (P,) and ptr[0] == 0
    for k in range(K):
        assert rows[ptr[k]:ptr[k + 1]].tolist() == [i for i in range(P) if label[i] == k]
    assert ptr[K] == sum(1 for l in label if 0 <= l < K) and np.all(rows[ptr[K]:] == -1)


def _brute_box(values):
    """min / max of float32 values by comparing their bytes as sign-magnitude integers: -0 < +0, NaN skipped"""
    keys = []
    for v in values:
        if v != v:
            continue
        b = struct.unpack("<i", struct.pack("<f", v))[0]
        keys.append((b if b >= 0 else -(b & 0x7FFFFFFF) - 1, v))
    if not keys:
        return np.float32(np.inf), np.float32(-np.inf)
    return min(keys)[1], max(keys)[1]


@pytest.mark.parametrize("name", ic.names())
def test_the_restatement_is_within_the_derived_bounds_of_exact_arithmetic(name):
    c = ic.case(name)
    ptr, rows, st = ic.reference(name)
    K = c["K"]
    xyz, f, w, hit = c["xyz"], c["features"], c["weight"], c["hit"]
    ex = ref.exact(ptr, rows, xyz, f, w)
    worst = 0.0

    def hold(got, value, bound, what):
        nonlocal worst
        if value is None:
            assert np.isnan(got), what
            return
        err = abs(float(got) - float(value)) if np.isfinite(got) else np.inf
        assert err <= bound, f"{what}: |{got} - {float(value)}| = {err} > {bound}"
        worst = max(worst, err / bound)

    for k in range(K):
        e = ex[k]
        m = rows[ptr[k]:ptr[k + 1]]
        n = len(m)
        # integers, exactly
        assert st["n"][k] == n == e["n"]
        for b in range(8):
            want = 0 if hit is None else sum(int(hit[i]) >> b & 1 for i in m)
            assert st["hits"][k, b] == want
        # lo / hi: equal to a brute force, bit for bit
        for a in range(3):
            lo, hi = _brute_box([xyz[i, a] for i in m])
            assert np.float32(lo).tobytes() == st["lo"][k, a].tobytes() and np.float32(hi).tobytes() == st["hi"][k, a].tobytes()
        # floats, within the bounds
        hold(st["wsum"][k], e["W"], ref.mean_bound(n, e["W"], e["W"]), f"wsum[{k}]")
        if e["W"] == 0:
            assert not st["centroid"][k].any() and not st["cov"][k].any() and (f is None or not st["feature"][k].any())
            continue
        for a in range(3):
            v = e["centroid"][a]
            hold(st["centroid"][k, a], v, None if v is None else ref.centroid_bound(n, v, e["absd"][a]), f"centroid[{k},{a}]")
        for q, (a, b) in enumerate(ref.PAIRS):
            v = e["cov"][q]
            hold(st["cov"][k, q], v, None if v is None else ref.cov_bound(n, v, e["absdd"][q], e["absd"][a], e["absd"][b]),
                 f"cov[{k},{q}]")
        for ch in range(0 if f is None else f.shape[1]):
            hold(st["feature"][k, ch], e["feature"][ch], ref.mean_bound(n, e["feature"][ch], e["absf"][ch]), f"feature[{k},{ch}]")
    print(f"{name}: worst |restatement - exact| / bound = {worst:.3f}")
    assert (st["feature"] is None) == (f is None)


def test_the_far_scene_does_not_cancel():
    """1000 units from the origin and 0.01 across: the covariance is around 1e-4 and comes out to float32 precision, where a sum
    of raw x x^T in float32 would have lost every digit of it"""
    c = ic.case("far_pivot")
    ptr, rows, st = ic.reference("far_pivot")
    ex = ref.exact(ptr, rows, c["xyz"], None, c["weight"])
    k = int(np.argmax(np.diff(ptr)))
    for q in (0, 3, 5):
        assert 1e-5 < float(ex[k]["cov"][q]) < 1e-3
        assert abs(float(st["cov"][k, q]) - float(ex[k]["cov"][q])) <= 2.0 ** -23 * float(ex[k]["cov"][q])


def test_twins_restate_to_identical_bits():
    a, b = ic.reference("twins")[2], ic.reference("twins_K3")[2]
    for key in ("n", "hits", "wsum", "centroid", "lo", "hi", "cov", "feature"):
        assert a[key][2].tobytes() == a[key][7].tobytes() == b[key][1].tobytes(), key


def test_vote_at_exact_ties_and_empty_instances():
    n = np.array([10, 10, 10, 0, 3, 7, 1], np.int32)
    hits = np.zeros((7, 8), np.int32)
    hits[:, 0] = [5, 4, 6, 0, 1, 7, 1]
    hits[:, 5] = [7, 0, 10, 0, 3, 0, 0]
    assert ref.vote(n, hits, 0.5).tolist() == [True, False, True, False, False, True, True]       # 5 / 10 == 0.5 is kept
    assert ref.vote(n, hits, 0.7, bit=5).tolist() == [True, False, True, False, True, False, False]  # 7 / 10 == 0.7, exactly
    assert ref.vote(n, hits, 1 / 3).tolist() == [True, True, True, False, True, True, True]       # the float next to 1 / 3: 1 of 3
    assert ref.vote(n, hits, 0.5, min_hits=6).tolist() == [False, False, True, False, False, True, False]
    assert ref.vote(n, hits, 0.0, min_hits=0).tolist() == [True] * 7                                # n = 0: 0 >= 0
    assert ref.vote(n, hits, 0.0, min_hits=1)[3] == False  # noqa: E712 -- an empty instance has no hit
    assert ref.fraction_of(0.7) == (7, 10) and ref.fraction_of(0.5) == (1, 2) and ref.fraction_of(1) == (1, 1)
    assert ref.rows_of(np.array([0, -1, 2, 7, -2 ** 31, 1], np.int32), np.array([True, False, True])).tolist() == [
        True, False, True, False, False, False]


# ---- the module's own checks (no GPU needed: every call below is refused first) -----------------------------------------------------
def test_module_surface_and_fraction():
    import goi_hyperplane_amd
    from goi_hyperplane_amd import instance, semantic
    assert goi_hyperplane_amd.instance is instance and "instance" in goi_hyperplane_amd.__all__
    assert instance.Members._fields == ("ptr", "rows", "K")
    assert instance.InstanceStats._fields == ("n", "hits", "wsum", "centroid", "lo", "hi", "cov", "feature", "members")
    assert callable(semantic.select_instances)
    for q in (0.5, 0.7, 0.1, 1 / 3, 0, 1, 0.999):
        assert instance.fraction_of(q) == ref.fraction_of(q)
    num, den = instance.fraction_of(1 / 3)
    assert den < 2 ** 32 and abs(num / den - 1 / 3) < 1e-9
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="0 <= min_fraction <= 1"):
            instance.fraction_of(bad)
    with pytest.raises(TypeError, match="min_fraction"):
        instance.fraction_of("half")


def test_argument_errors_name_dtype_and_shape_first_then_the_device():
    from goi_hyperplane_amd import instance
    label = torch.zeros(10, dtype=torch.int32)
    xyz = torch.zeros(10, 3)
    with pytest.raises(TypeError, match="label must be int32"):
        instance.members(label.long(), 2)
    with pytest.raises(ValueError, match=r"label must have shape \(P,\)"):
        instance.members(label.reshape(2, 5), 2)
    with pytest.raises(TypeError, match="capacity must be an int or None"):
        instance.members(label, 2.0)
    with pytest.raises(ValueError, match="0 <= capacity < 2\\^30"):
        instance.members(label, -1)
    with pytest.raises(ValueError, match="0 <= capacity < 2\\^30"):
        instance.members(label, 2 ** 30)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        instance.members(label, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        instance.members(label)
    with pytest.raises(TypeError, match="xyz must be float32"):
        instance.stats(label, xyz.double(), capacity=2)
    with pytest.raises(ValueError, match=r"xyz must have shape \(10, 3\)"):
        instance.stats(label, xyz[:9], capacity=2)
    with pytest.raises(ValueError, match="features must have shape \\(10, S\\) with 1 <= S <= 32"):
        instance.stats(label, xyz, features=torch.zeros(10, 33), capacity=2)
    with pytest.raises(ValueError, match="features must have shape"):
        instance.stats(label, xyz, features=torch.zeros(10, 0), capacity=2)
    with pytest.raises(TypeError, match="weight must be float32"):
        instance.stats(label, xyz, weight=torch.zeros(10, dtype=torch.float64), capacity=2)
    with pytest.raises(TypeError, match="hit must be bool or uint8"):
        instance.stats(label, xyz, hit=torch.zeros(10, dtype=torch.int32), capacity=2)
    with pytest.raises(TypeError, match="members must be what members\\(\\) returned"):
        instance.stats(label, xyz, members=(label, label))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        instance.stats(label, xyz, capacity=2)
    with pytest.raises(TypeError, match="stats must be what stats\\(\\) returned"):
        instance.vote((1, 2))
    with pytest.raises(TypeError, match="keep must be bool"):
        instance.rows_of(label, torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        instance.rows_of(label, torch.zeros(3, dtype=torch.bool))
    with pytest.raises(TypeError, match="hit must be bool"):
        instance.select(label, torch.zeros(10, dtype=torch.uint8), capacity=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        instance.select(label, torch.zeros(10, dtype=torch.bool), capacity=2)
