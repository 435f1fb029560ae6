"""Plain numpy references and result checkers for the device-wide radix sort and exclusive scan (csrc/scan_sort.hip).

Shared by tests/test_gpu_scan_sort.py, which feeds them device results, and tests/test_scan_sort_cpu.py, which feeds
them deliberately wrong results to show that every check can fail.  Arrays are uint32 (device int32 buffers are
viewed as uint32).
"""
from __future__ import annotations

import numpy as np

SENTINEL = np.uint32(0xDEADBEEF)  # written past the count before a call; must still be there afterwards


def pass_plan(lo: int, hi: int) -> list[tuple[int, int]]:
    """(shift, nbits) of each pass: [lo, hi) in the fewest passes of at most 8 bits, split as evenly as possible, the
    wider passes first (the split radix_sort_pairs makes; a caller-supplied histogram must follow it)."""
    bits = hi - lo
    passes = (bits + 7) // 8
    plan, sh = [], lo
    for p in range(passes):
        nb = (bits - (sh - lo) + (passes - p) - 1) // (passes - p)
        plan.append((sh, nb))
        sh += nb
    return plan


def digits(keys: np.ndarray, lo: int, hi: int) -> np.ndarray:
    k = np.asarray(keys, dtype=np.uint32).astype(np.uint64)
    return ((k >> np.uint64(lo)) & np.uint64((1 << (hi - lo)) - 1)).astype(np.uint32)


def digit_histograms(keys: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """[passes][256] uint32: per pass, how many keys hold each digit value."""
    k = np.asarray(keys, dtype=np.uint32)
    out = np.zeros((len(pass_plan(lo, hi)), 256), dtype=np.uint32)
    for p, (sh, nb) in enumerate(pass_plan(lo, hi)):
        out[p, :1 << nb] = np.bincount(digits(k, sh, sh + nb), minlength=1 << nb)
    return out


def reference_perm(keys: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """The stable ascending order of `keys` by bits [lo, hi)."""
    d = digits(keys, lo, hi)
    if hi - lo <= 16:
        d = d.astype(np.uint16)  # (same order; numpy sorts 16-bit keys with a radix sort)
    return np.argsort(d, kind="stable").astype(np.uint32)


def _first_diff(a: np.ndarray, b: np.ndarray) -> str:
    i = int(np.flatnonzero(a != b)[0])
    return f"first difference at {i} of {len(a)}: got {int(a[i]):#010x}, want {int(b[i]):#010x}"


def check_sort(keys_in: np.ndarray, lo: int, hi: int, keys_out: np.ndarray, vals_out: np.ndarray) -> None:
    """The sort's output for input keys `keys_in` and values iota: the values must be the stable order exactly, the
    keys the input keys in that order in all 32 bits (bits outside [lo, hi) travel with their key)."""
    keys_in = np.asarray(keys_in, dtype=np.uint32)
    n = len(keys_in)
    assert len(keys_out) == n and len(vals_out) == n, (len(keys_out), len(vals_out), n)
    perm = reference_perm(keys_in, lo, hi)
    vals_out = np.asarray(vals_out, dtype=np.uint32)
    keys_out = np.asarray(keys_out, dtype=np.uint32)
    if not np.array_equal(vals_out, perm):
        raise AssertionError("sorted values are not the stable order: " + _first_diff(vals_out, perm))
    want = keys_in[perm]
    if not np.array_equal(keys_out, want):
        raise AssertionError("sorted keys differ: " + _first_diff(keys_out, want))


def check_untouched(name: str, buf: np.ndarray, count: int) -> None:
    """Positions count .. len(buf) still hold the sentinel."""
    tail = np.asarray(buf, dtype=np.uint32)[count:]
    bad = np.flatnonzero(tail != SENTINEL)
    if len(bad):
        i = int(bad[0]) + count
        raise AssertionError(f"{name}[{i}] was written past the count {count}: {int(buf[i]):#010x}")


def scan_reference(values: np.ndarray, gather: np.ndarray | None, count: int) -> tuple[np.ndarray, int]:
    """(exclusive prefix sums mod 2^32 [count], total mod 2^32) of f(j) = values[gather[j]] or values[j], j < count."""
    v = np.asarray(values, dtype=np.uint32)
    f = v[np.asarray(gather, dtype=np.int64)[:count]] if gather is not None else v[:count]
    inc = np.cumsum(f.astype(np.uint64), dtype=np.uint64)
    excl = np.zeros(count, dtype=np.uint64)
    excl[1:] = inc[:-1]
    total = int(inc[-1]) if count else 0
    return (excl & np.uint64(0xFFFFFFFF)).astype(np.uint32), total & 0xFFFFFFFF


def check_scan(values: np.ndarray, gather: np.ndarray | None, count: int, out: np.ndarray,
               total: int | None = None) -> None:
    want, want_total = scan_reference(values, gather, count)
    out = np.asarray(out, dtype=np.uint32)[:count]
    if not np.array_equal(out, want):
        raise AssertionError("exclusive scan differs: " + _first_diff(out, want))
    if total is not None and int(total) != want_total:
        raise AssertionError(f"scan total {int(total):#x} != {want_total:#x}")
