"""CPU checks that keep tests/test_gpu_scan_sort.py honest (no GPU needed):
  * its checkers fail on each kind of subtly wrong result a broken sort or scan would produce;
  * its size tables straddle every size at which csrc/scan_sort.hip changes shape, tile count, look-back or scan
    path -- recomputed from the constants in the kernel source, so retuning one fails here instead of silently losing
    coverage;
  * the entry points refuse bad arguments (and sorts of 2^30 keys or more) before any HIP call.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import test_gpu_scan_sort as G
from tests.scan_sort_reference import (SENTINEL, check_scan, check_sort, check_untouched, digit_histograms, pass_plan,
                                       reference_perm, scan_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "scan_sort.hip")).read()


# ---- the checkers are sensitive ------------------------------------------------------------------------------------
def _sorted_pair(keys, lo, hi):
    perm = reference_perm(keys, lo, hi)
    return keys[perm].copy(), perm.copy()


@pytest.fixture
def keys():
    rng = np.random.default_rng(7)
    return rng.integers(0, 2 ** 32, 5000, dtype=np.uint32) & np.uint32(0xFFFF0F0F)  # many equal digits in [0, 12)


def test_check_sort_accepts_the_reference(keys):
    for lo, hi in ((0, 32), (0, 12), (4, 9), (0, 1)):
        k, v = _sorted_pair(keys, lo, hi)
        check_sort(keys, lo, hi, k, v)


def test_check_sort_rejects_an_unstable_swap(keys):
    k, v = _sorted_pair(keys, 0, 12)
    d = (k & 0xFFF)
    i = int(np.flatnonzero(d[1:] == d[:-1])[0])  # two neighbours with equal digits: swapping them is still "sorted"
    k[[i, i + 1]], v[[i, i + 1]] = k[[i + 1, i]], v[[i + 1, i]]
    assert np.all(np.diff((k & 0xFFF).astype(np.int64)) >= 0)
    with pytest.raises(AssertionError, match="stable order"):
        check_sort(keys, 0, 12, k, v)


def test_check_sort_rejects_a_duplicate_and_a_drop(keys):
    k, v = _sorted_pair(keys, 0, 32)
    k[10], v[10] = k[11], v[11]
    with pytest.raises(AssertionError):
        check_sort(keys, 0, 32, k, v)


def test_check_sort_rejects_a_changed_bit_outside_the_range(keys):
    k, v = _sorted_pair(keys, 0, 12)
    k[100] ^= np.uint32(1 << 31)
    with pytest.raises(AssertionError, match="sorted keys differ"):
        check_sort(keys, 0, 12, k, v)
    k, v = _sorted_pair(keys, 4, 9)
    k[5] ^= np.uint32(1)  # below lo
    with pytest.raises(AssertionError, match="sorted keys differ"):
        check_sort(keys, 4, 9, k, v)


def test_check_untouched_rejects_a_write_past_the_count():
    buf = np.full(100, SENTINEL, dtype=np.uint32)
    buf[:60] = 0
    check_untouched("keys1", buf, 60)
    buf[99] = 0
    with pytest.raises(AssertionError, match=r"keys1\[99\]"):
        check_untouched("keys1", buf, 60)


def test_check_scan_rejects_inclusive_wrong_total_and_no_wrap():
    rng = np.random.default_rng(3)
    v = rng.integers(0, 2 ** 32, 3000, dtype=np.uint32)
    g = rng.permutation(3000)
    want, total = scan_reference(v, g, 3000)
    check_scan(v, g, 3000, want, total)
    inclusive = (np.cumsum(v[g].astype(np.uint64)) & 0xFFFFFFFF).astype(np.uint32)
    with pytest.raises(AssertionError, match="exclusive scan differs"):
        check_scan(v, g, 3000, inclusive)
    with pytest.raises(AssertionError, match="total"):
        check_scan(v, g, 3000, want, total + 2 ** 32)
    with pytest.raises(AssertionError, match="exclusive scan differs"):  # the gather ignored
        check_scan(v, g, 3000, scan_reference(v, None, 3000)[0])
    assert int(np.cumsum(v[g].astype(np.uint64))[-1]) >= 2 ** 32  # (the case wraps)


def test_pass_plan_and_histograms():
    assert pass_plan(0, 32) == [(0, 8), (8, 8), (16, 8), (24, 8)]
    assert pass_plan(0, 15) == [(0, 8), (8, 7)]
    assert pass_plan(0, 30) == [(0, 8), (8, 8), (16, 7), (23, 7)]
    assert pass_plan(0, 31) == [(0, 8), (8, 8), (16, 8), (24, 7)]
    assert pass_plan(5, 6) == [(5, 1)]
    k = np.array([0x0102, 0x0201, 0x0102, 0xFFFF], dtype=np.uint32)
    h = digit_histograms(k, 0, 15)
    assert h.shape == (2, 256) and h[0, 2] == 2 and h[0, 1] == 1 and h[0, 255] == 1 and h[1, 0x7F] == 1
    assert h.sum(1).tolist() == [4, 4]


@pytest.mark.parametrize("dist", ["uniform", "depth", "tile", "equal", "lowbyte", "highbyte", "two", "ascending",
                                  "descending", "junk"])
def test_key_distributions(dist):
    """The generators make what their names promise (run on the CPU here; the GPU module runs them on the device)."""
    lo, hi = (0, 15) if dist == "tile" else (0, 14) if dist == "junk" else (0, 32)
    g = torch.Generator().manual_seed(1)
    k = G.make_keys(dist, 100_000, lo, hi, g, device="cpu").numpy().view(np.uint32)
    assert k.shape == (100_000,)
    if dist == "depth":
        pad = k == 0xFFFFFFFF
        assert 0.3 <= pad.mean() <= 0.5
        z = k[~pad].view(np.float32)
        assert z.min() >= 0.2 and z.max() <= 20.0
    elif dist == "tile":
        assert k.max() < 2 ** 15 and np.sort(np.bincount(k))[-6:].sum() >= 0.88 * len(k)
    elif dist == "equal":
        assert len(np.unique(k)) == 1
    elif dist == "lowbyte":
        assert len(np.unique(k >> 8)) == 1 and len(np.unique(k & 0xFF)) == 256
    elif dist == "highbyte":
        assert len(np.unique(k & 0xFFFFFF)) == 1 and len(np.unique(k >> 24)) == 256
    elif dist == "two":
        assert len(np.unique(k)) == 2
    elif dist == "ascending":
        assert np.all(np.diff(k.astype(np.int64)) > 0)
    elif dist == "descending":
        assert np.all(np.diff(k.astype(np.int64)) < 0)
    elif dist == "junk":
        assert len(np.unique(k >> 14)) > 1000 and (k & 0x3FFF).max() > 0
    else:
        assert len(np.unique(k >> 24)) == 256


# ---- the size tables track the kernel ------------------------------------------------------------------------------
def _const(name):
    m = re.search(rf"constexpr\s+\w+\s+{name}\s*=\s*(\d+)\s*;", SRC)
    assert m, name
    return int(m.group(1))


def kernel_constants():
    c = {
        "SWEEP_TARGET_TILES": _const("SWEEP_TARGET_TILES"),
        "SWEEP_GROUPED_MAX_TILES": _const("SWEEP_GROUPED_MAX_TILES"),
        "GOI_SORT_THREADS": int(re.search(r"#define GOI_SORT_THREADS (\d+)", SRC).group(1)),
        "SORT_ITEMS": _const("SORT_ITEMS"),
        "SCAN_CHUNK": _const("SCAN_THREADS") * _const("SCAN_ITEMS"),
    }
    a = re.search(r"sweep_adaptive\(size_t n\) \{ return n > \(\(size_t\)(\d+) << (\d+)\)", SRC)
    c["ADAPTIVE"] = int(a.group(1)) << int(a.group(2))
    assert f"n <= ((size_t){a.group(1)} << {a.group(2)})" in SRC  # sweep_min_items_for: the same bound
    c["STATUS_ROWS"] = int(re.search(r"/ \(\(size_t\)512 \* items\) > (\d+)\) items <<= 1", SRC).group(1))
    shapes = re.findall(r"sweep_pass_k<(\d+), (\d+)><<<", SRC)
    assert len(shapes) == 2
    (c["FIXED_THREADS"], c["FIXED_ITEMS"]), (c["ADAPT_THREADS"], c["ADAPT_ITEMS"]) = [tuple(map(int, s)) for s in shapes]
    c["GROUP_LOG0"] = int(re.search(r"uint32_t gs_log = (\d+);", SRC).group(1))
    c["RAW_CHUNKS"] = int(re.search(r"const bool raw = total == nullptr && nb <= (\d+);", SRC).group(1))
    c["CARRY_CHUNKS"] = int(re.search(r"__launch_bounds__\((\d+)\) void scan_partials_k", SRC).group(1))
    return c


def thresholds(c):
    """{name: (threshold, tile or None)} in keys.  Capacity thresholds apply to sorts whose count is their capacity."""
    at, ai = c["ADAPT_THREADS"], c["ADAPT_ITEMS"]
    big_tile = at * ai
    fixed_tile = c["FIXED_THREADS"] * c["FIXED_ITEMS"]
    return {
        "wave": (64, None),
        "fixed tile (1024 x 4)": (fixed_tile, None),
        "histogram / three-kernel block (SORT_TILE)": (c["GOI_SORT_THREADS"] * c["SORT_ITEMS"], None),
        "group size 16 -> 32 (1024 x 4 tiles)": ((1 << (2 * c["GROUP_LOG0"])) * fixed_tile, fixed_tile),
        "adaptive tile above": (c["ADAPTIVE"], None),
        "min_items 4 -> 8": (at * 4 * c["STATUS_ROWS"], None),
        "min_items 8 -> 16 (non-adaptive 512 x 16)": (at * 8 * c["STATUS_ROWS"], None),
        "grouped -> chained look-back (8192-key tiles)": (c["SWEEP_GROUPED_MAX_TILES"] * big_tile, big_tile),
    }


def count_thresholds(c):
    """Keys per thread chosen on the device from the count: at most SWEEP_TARGET_TILES tiles."""
    at, tt = c["ADAPT_THREADS"], c["SWEEP_TARGET_TILES"]
    return {"items 16 vs 8": at * 8 * tt, "items 8 vs 4": at * 4 * tt, "items 4 vs 2 (sort_small)": at * 2 * tt}


def test_kernel_constants_parse():
    c = kernel_constants()
    assert c["SCAN_CHUNK"] == 2048 and c["ADAPTIVE"] == 2 << 20 and c["ADAPT_ITEMS"] == c["SORT_ITEMS"]
    assert c["FIXED_ITEMS"] < c["ADAPT_ITEMS"]


def _default_caps(dist_ok=lambda d: True):
    return {c.cap for c in G.SORT_CASES if not c.opts and c.count is None and dist_ok(c.dist)}


def test_sort_table_straddles_every_capacity_threshold():
    c = kernel_constants()
    real = _default_caps(lambda d: d not in G.TRIVIAL_DISTS)  # (a trivial pass skips the look-back)
    for name, (t, tile) in thresholds(c).items():
        need = {t - 1, t, t + 1} | ({t - tile, t + tile} if tile else set())
        assert need <= real, f"{name}: no default case at {sorted(need - real)}"


def test_sort_table_straddles_the_device_count_thresholds():
    c = kernel_constants()
    th = count_thresholds(c)
    a = c["ADAPTIVE"]
    counted = {(x.cap, x.count) for x in G.SORT_CASES if x.count is not None and not x.opts}
    small = {(x.cap, x.count) for x in G.SORT_CASES if x.count is not None and x.opts == G.SMALL}
    for name in ("items 16 vs 8", "items 8 vs 4"):
        t = th[name]
        caps = {cap for cap, _ in counted if cap > a}
        assert any({(cap, t - 1), (cap, t), (cap, t + 1)} <= counted for cap in caps), name
    t = th["items 4 vs 2 (sort_small)"]
    assert any({(cap, t), (cap, t + 1)} <= small for cap, _ in small), "sort_small count threshold"
    assert {t - 1, t, t + 1} <= {x.cap for x in G.SORT_CASES if x.opts == G.SMALL and x.count is None}
    # count 0 and 1 under a capacity, count = capacity on the device, a close-up (count far below capacity)
    assert {cnt for _, cnt in counted} >= {0, 1}
    assert any(cap == cnt and cap > a for cap, cnt in counted)
    assert any(cap >= 4 * a and cnt * 16 < cap for cap, cnt in counted)


def test_option_subsets_cross_their_own_thresholds():
    c = kernel_constants()
    th = thresholds(c)
    v0 = {x.cap for x in G.SORT_CASES if x.opts == G.V0}
    t = th["histogram / three-kernel block (SORT_TILE)"][0]
    assert {0, 1, t - 1, t, t + 1} <= v0
    chain = {x.n for x in G.SORT_CASES if x.opts == G.CHAIN}
    grouped_max = th["grouped -> chained look-back (8192-key tiles)"][0]
    assert any(th["group size 16 -> 32 (1024 x 4 tiles)"][0] < n < th["adaptive tile above"][0] for n in chain)
    assert any(n > grouped_max for n in chain) and any(n < grouped_max for n in chain)
    assert any(x.ghist for x in G.SORT_CASES) and any(x.flags & 1 for x in G.SORT_CASES)
    assert any(x.ghist and x.count is not None and x.count < x.cap for x in G.SORT_CASES)


def test_sort_table_covers_bit_ranges_and_distributions():
    ranges = {(x.lo, x.hi) for x in G.SORT_CASES}
    assert {(0, 32), (0, 15), (0, 14), (0, 30), (0, 31), (0, 8), (0, 1)} <= ranges
    assert any(lo > 0 for lo, _ in ranges)
    assert {x.dist for x in G.SORT_CASES} == {"uniform", "depth", "tile", "equal", "lowbyte", "highbyte", "two",
                                               "ascending", "descending", "junk"}
    assert max(x.cap for x in G.SORT_CASES) <= 20_000_000  # (numpy references stay at <= 20 M keys)


def test_scan_table_straddles_its_thresholds():
    c = kernel_constants()
    chunk = c["SCAN_CHUNK"]
    plain = {x.cap for x in G.SCAN_CASES if x.count is None and not x.inplace}
    assert {0, 1, chunk - 1, chunk, chunk + 1} <= plain
    carry = c["CARRY_CHUNKS"] * chunk
    with_total = {x.cap for x in G.SCAN_CASES if x.total and x.count is None}
    assert {carry - 1, carry, carry + 1} <= with_total
    raw = c["RAW_CHUNKS"] * chunk
    no_total = {x.cap for x in G.SCAN_CASES if not x.total and x.count is None}
    assert {raw - 1, raw, raw + 1} <= no_total
    assert any(x.gather == "perm" for x in G.SCAN_CASES) and any(x.gather == "repeat" for x in G.SCAN_CASES)
    assert any(x.gather and not x.inplace for x in G.SCAN_CASES)  # (the stash path)
    assert any(x.inplace and not x.gather for x in G.SCAN_CASES)
    assert any(x.count is not None and x.count < x.cap for x in G.SCAN_CASES)
    assert any(x.wide for x in G.SCAN_CASES)


# ---- host refusals (they return before any HIP call) -----------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.goi_raster_last_error().decode()


FAKE = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first


@pytest.mark.parametrize("n,lo,hi", [(-1, 0, 32), (1 << 30, 0, 32), (100, -1, 8), (100, 0, 33), (100, 8, 8), (100, 9, 8)])
def test_sort_refuses_bad_sizes_and_ranges(lib, n, lo, hi):
    assert lib.goi_raster_debug_sort_pairs(None, None, None, None, n, lo, hi, None, None, 0, None, None, None) < 0
    assert "goi_raster_debug_sort_pairs" in _err(lib)
    assert lib.goi_raster_debug_sort_workspace_bytes(n, lo, hi) == 0


def test_sort_workspace_bytes(lib):
    assert lib.goi_raster_debug_sort_workspace_bytes(0, 0, 32) > 0
    assert lib.goi_raster_debug_sort_workspace_bytes((1 << 30) - 1, 0, 32) > lib.goi_raster_debug_sort_workspace_bytes(1 << 20, 0, 32)


def test_sort_refuses_device_count_and_histograms_without_onesweep(lib):
    from goi_hyperplane_amd import _lib
    before = _lib.OPTIONS.get("sort_variant", 1)
    try:
        _lib.set_option("sort_variant", 0)
        for n_dev, gh in ((FAKE, None), (None, FAKE)):
            assert lib.goi_raster_debug_sort_pairs(FAKE, FAKE, FAKE, FAKE, 100, 0, 32, n_dev, gh, 0, None, FAKE, None) < 0
            assert "onesweep" in _err(lib)
    finally:
        _lib.set_option("sort_variant", before)
    assert lib.goi_raster_debug_sort_pairs(FAKE, FAKE, FAKE, FAKE, 100, 0, 32, None, None, 2, None, FAKE, None) < 0
    assert "flags" in _err(lib)
    assert lib.goi_raster_debug_sort_pairs(None, None, None, None, 0, 0, 32, None, None, 0, None, None, None) == 0  # (nothing to do)
    assert lib.goi_raster_debug_sort_pairs(None, None, None, None, 100, 0, 32, None, None, 0, None, None, None) < 0
    assert "NULL" in _err(lib)


def test_scan_refuses_in_place_with_a_gather(lib):
    assert lib.goi_raster_debug_exclusive_scan(FAKE, C.c_void_p(1 << 21), FAKE, 100, None, None, FAKE, None) < 0
    assert "data race" in _err(lib)
    assert lib.goi_raster_debug_exclusive_scan(FAKE, None, FAKE, -1, None, None, FAKE, None) < 0
    assert lib.goi_raster_debug_exclusive_scan(FAKE, None, FAKE, 1 << 32, None, None, FAKE, None) < 0
    assert lib.goi_raster_debug_exclusive_scan(None, None, None, 100, None, None, None, None) < 0
    assert "NULL" in _err(lib)
    assert lib.goi_raster_debug_scan_workspace_bytes(-1) == 0 and lib.goi_raster_debug_scan_workspace_bytes(0) > 0


def test_knn_and_dbscan_refuse_two_to_the_thirty_points(lib):
    """The onesweep status words carry 30-bit counts: both callers of the sort refuse 2^30 keys or more."""
    assert lib.goi_knn_dist2(1 << 30, None, None, None, None) < 0 and "2^30" in _err(lib)
    assert lib.goi_knn_workspace_bytes(1 << 30) == 0 and lib.goi_knn_workspace_bytes((1 << 30) - 1) > 0
    assert lib.goi_semantic_dbscan(1 << 30, None, 0.35, 600, None, None, FAKE, None, None) < 0 and "2^30" in _err(lib)
    assert lib.goi_semantic_dbscan_workspace_bytes(1 << 30) == 0
    assert lib.goi_semantic_dbscan_workspace_bytes((1 << 30) - 1) > 0
    huge = torch.zeros(1, 3).expand(1 << 30, 3)  # (no memory behind it: refused before anything looks at the data)
    from goi_hyperplane_amd import cluster, knn
    with pytest.raises(ValueError, match=r"2\^30"):
        cluster.dbscan(huge, eps=0.35, min_samples=600)
    with pytest.raises(RuntimeError, match=r"2\^30"):
        knn.distCUDA2(huge)
