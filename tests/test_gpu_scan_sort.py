"""The device-wide radix sort and exclusive scan (csrc/scan_sort.hip) called directly, against numpy.

Every sort and scan of the product goes through these two primitives: the depth and tile sorts and the scan over
tiles_touched of the rasterizer, the Morton-code sort of k-NN, the cell-key sorts and head scans of DBSCAN.  The
entry points goi_raster_debug_sort_pairs / goi_raster_debug_exclusive_scan (include/goi_raster.h) run them on
caller buffers with the product's calling conventions: a count on the device below the capacity the grids were sized
for, caller-supplied digit histograms, caller-cleared control words.

The reference is numpy: np.argsort(kind="stable") of the digits for the sort (values are iota, so the value output
must BE the permutation), np.cumsum in uint64 masked to 32 bits for the scan.  Positions past the count hold a
sentinel that must survive.  The size tables straddle every size at which the kernels change shape, tile count,
look-back kind or scan path; tests/test_scan_sort_cpu.py recomputes those sizes from the constants in
scan_sort.hip and fails when a table no longer straddles one.
"""
from __future__ import annotations

import ctypes as C
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from tests.scan_sort_reference import (SENTINEL, check_scan, check_sort, check_untouched, digit_histograms,
                                       pass_plan)

pytestmark = pytest.mark.gpu

SENT_I32 = int(SENTINEL.view(np.int32))
DEFAULT_OPTIONS = {"sort_variant": 1, "sort_small": 0, "sort_lookback": 1}
TRIVIAL_DISTS = ("equal", "lowbyte", "highbyte")  # every pass, or every pass but one, has a single digit


@dataclass(frozen=True)
class SortCase:
    cap: int                 # n: the capacity grids, buffers and control words are sized for
    dist: str = "uniform"
    lo: int = 0
    hi: int = 32
    count: int | None = None  # not None: the count lives on the device (n_dev) and may be below cap
    opts: tuple = ()          # (name, value) options for this case
    ghist: bool = False       # caller-supplied digit histograms (the rasterizer's convention)
    flags: int = 0            # 1: the caller zeroed the workspace

    @property
    def n(self) -> int:
        return self.cap if self.count is None else self.count

    @property
    def id(self) -> str:
        s = f"{self.cap}" if self.count is None else f"{self.count}of{self.cap}"
        s += f"-{self.dist}-{self.lo}_{self.hi}"
        s += "".join(f"-{k}{v}" for k, v in self.opts)
        return s + ("-ghist" if self.ghist else "") + ("-cleared" if self.flags & 1 else "")


S = SortCase
M = 1 << 20

# ---- default options, count = capacity (host-sized sorts: k-NN, DBSCAN, the exact forward) -------------------------
SORT_DEFAULT = [
    S(0), S(1), S(1, "depth"),
    S(63, "depth"), S(64, "tile", 0, 15), S(65),                                    # one wave
    S(4095, "two"), S(4096, "uniform", 0, 30), S(4097, "depth"),                    # one 1024 x 4 tile
    S(8191, "tile", 0, 15), S(8192, "uniform", 0, 31), S(8193, "ascending"),        # SORT_TILE: histogram blocks
    S(8193, "uniform", 0, 8), S(8193, "uniform", 0, 1), S(8193, "equal"),
    S(65535, "descending"), S(65536, "junk", 0, 14), S(65537, "uniform", 5, 27),
    S(65537, "lowbyte"), S(65537, "highbyte"),
    # 1024 x 4 tiles: groups of 16 up to 256 tiles, of 32 above
    S(M - 4096, "depth"), S(M - 1, "depth"), S(M, "tile", 0, 15), S(M + 1, "uniform"), S(M + 4096, "two"),
    # adaptive 512 x (2..16) above 2 M, min_items 4
    S(2 * M - 1, "depth"), S(2 * M, "tile", 0, 15), S(2 * M + 1, "depth"), S(2 * M + 1, "lowbyte"),
    # min_items 4 -> 8
    S(4 * M - 1, "uniform", 0, 30), S(4 * M, "depth"), S(4 * M + 1, "tile", 0, 15),
    # 8192-key tiles: grouped look-back up to 640 tiles, chained above
    S(5 * M - 8192, "depth"), S(5 * M - 1, "tile", 0, 15), S(5 * M, "uniform", 0, 31), S(5 * M + 1, "depth"),
    S(5 * M + 8192, "descending"), S(5 * M + 1, "highbyte"),
    # min_items 8 -> 16: the 512 x 16 kernel is no longer adaptive (early tickets)
    S(8 * M - 1, "depth"), S(8 * M, "tile", 0, 15), S(8 * M + 1, "uniform"), S(8 * M + 1, "equal"),
    S(20_000_000, "depth"),
]

# ---- default options, count on the device (the speculative forward's tile sort, the depth sort of the listed) -------
SORT_COUNTED = [
    S(M, count=0), S(M, count=1), S(65537, "depth", count=65536),
    S(4 * M, "depth", count=4 * M),
    S(8 * M, "depth", count=240_000),                                   # close-up: 30 tiles of a large capacity
    # keys per thread chosen on the device under min_items 4: 4 up to 1 M keys, 8 up to 2 M, 16 above
    S(4 * M, "tile", 0, 15, count=M - 1), S(4 * M, "depth", count=M), S(4 * M, "two", count=M + 1),
    S(4 * M, "depth", count=2 * M - 1), S(4 * M, "tile", 0, 15, count=2 * M), S(4 * M, "uniform", count=2 * M + 1),
    # non-adaptive 512 x 16 with the count below the capacity: blocks past it hold tickets and leave
    S(20_000_000, "depth", count=5 * M + 1), S(20_000_000, "tile", 0, 15, count=3_000_000),
]

# ---- caller-supplied histograms (every rasterizer sort) and caller-cleared control words ---------------------------
SORT_CALLER = [
    S(8193, "depth", ghist=True), S(65537, "equal", ghist=True), S(M, "depth", count=500_000, ghist=True),
    S(4 * M, "tile", 0, 15, count=2 * M + 1, ghist=True), S(5 * M + 1, "depth", ghist=True),
    S(8 * M, "tile", 0, 15, count=6 * M, ghist=True), S(M, count=0, ghist=True),
    S(8193, "two", flags=1), S(2 * M + 1, "depth", flags=1), S(5 * M + 1, "tile", 0, 15, flags=1),
]

V0 = (("sort_variant", 0),)
SMALL = (("sort_small", 1),)
CHAIN = (("sort_lookback", 0),)
SORT_OPTIONS = [
    # the three-kernel sort: histogram / scan / scatter per pass
    S(0, opts=V0), S(1, opts=V0), S(65, opts=V0), S(8191, "depth", opts=V0), S(8192, "tile", 0, 15, opts=V0),
    S(8193, "uniform", 0, 30, opts=V0), S(65537, "junk", 0, 14, opts=V0), S(M + 1, "lowbyte", opts=V0),
    S(2 * M + 1, "depth", opts=V0), S(8 * M + 1, "uniform", 0, 31, opts=V0),
    # sort_small: the adaptive tile below 2 M keys too (min_items 2: keys per thread 2 up to 512 K keys, 4 above)
    S(65, opts=SMALL), S(8193, "depth", opts=SMALL), S(M // 2 - 1, "tile", 0, 15, opts=SMALL),
    S(M // 2, "depth", opts=SMALL), S(M // 2 + 1, "two", opts=SMALL), S(2 * M, "depth", opts=SMALL),
    S(2 * M, "depth", count=M // 2, opts=SMALL), S(2 * M, "tile", 0, 15, count=M // 2 + 1, opts=SMALL),
    S(2 * M, count=0, opts=SMALL), S(4 * M + 1, "depth", count=M + 1, opts=SMALL),
    # the chained look-back everywhere, the grouped range included
    S(65537, "depth", opts=CHAIN), S(M + 1, "tile", 0, 15, opts=CHAIN), S(2 * M + 1, "depth", opts=CHAIN),
    S(4 * M, "uniform", count=M + 1, opts=CHAIN), S(5 * M + 1, "depth", opts=CHAIN),
    S(8 * M + 1, "tile", 0, 15, opts=CHAIN),
]

SORT_CASES = SORT_DEFAULT + SORT_COUNTED + SORT_CALLER + SORT_OPTIONS


@dataclass(frozen=True)
class ScanCase:
    cap: int
    count: int | None = None  # not None: n_dev
    gather: str | None = None  # "perm" | "repeat"
    inplace: bool = False
    total: bool = False
    wide: bool = False         # 32-bit values: the sums wrap 2^32

    @property
    def n(self) -> int:
        return self.cap if self.count is None else self.count

    @property
    def id(self) -> str:
        s = f"{self.cap}" if self.count is None else f"{self.count}of{self.cap}"
        return (s + (f"-{self.gather}" if self.gather else "") + ("-inplace" if self.inplace else "")
                + ("-total" if self.total else "") + ("-wide" if self.wide else ""))


T = ScanCase
SCAN_CASES = [
    T(0), T(0, total=True), T(1, total=True), T(1, gather="perm"),
    T(2047), T(2048, total=True), T(2049, wide=True), T(2049, gather="perm", total=True),
    T(2049, gather="repeat", wide=True), T(2049, inplace=True, wide=True),
    # the block sums scanned by scan_partials_k (a total is wanted): its carry loop runs past 1024 chunks
    T(2 * M - 1, total=True, wide=True), T(2 * M, total=True), T(2 * M + 1, total=True, wide=True),
    T(2 * M + 1, gather="perm", total=True),
    # no total: raw block sums up to 4096 chunks, scan_partials_k above
    T(8 * M - 1, wide=True), T(8 * M), T(8 * M + 1, wide=True), T(8 * M + 1, gather="repeat"),
    T(8 * M + 1, gather="perm", wide=True), T(8 * M + 1, inplace=True, wide=True),
    # the count on the device
    T(4 * M, count=1_000_001, total=True, wide=True), T(4 * M, count=0, total=True),
    T(8 * M + 1, count=8 * M, gather="perm"), T(8 * M + 1, count=2049, inplace=True), T(M, count=M - 1, gather="repeat"),
]


# ---- helpers --------------------------------------------------------------------------------------------------------
def _lib():
    from goi_hyperplane_amd import _lib as L
    return L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _gen(tag: str) -> torch.Generator:
    g = torch.Generator(device="cuda")
    g.manual_seed(zlib.crc32(tag.encode()))
    return g


def _i32(x: torch.Tensor) -> torch.Tensor:
    """int64 values in [0, 2^32) -> int32 with the same 32 bits."""
    return torch.where(x >= 2 ** 31, x - 2 ** 32, x).to(torch.int32)


def make_keys(dist: str, n: int, lo: int, hi: int, g: torch.Generator, device="cuda") -> torch.Tensor:
    """int32 [n] keys (uint32 bit patterns) of a named distribution, generated on `device` from `g`."""
    def ri(a, b, size=(n,)):
        return torch.randint(a, b, size, generator=g, device=device, dtype=torch.int64)

    def rand():
        return torch.rand(n, generator=g, device=device)

    if dist == "uniform":
        return _i32(ri(0, 2 ** 32))
    if dist == "depth":  # float32 bits of view-space depths, 40 % culled pads
        z = (rand() * 19.8 + 0.2).to(torch.float32).view(torch.int32)
        return torch.where(rand() < 0.4, torch.full_like(z, -1), z)
    if dist == "tile":  # tile ids, 90 % of them in six hot tiles
        hot = ri(0, 1 << (hi - lo), (6,))
        ids = torch.where(rand() < 0.9, hot[ri(0, 6)], ri(0, 1 << (hi - lo)))
        return _i32(ids << lo)
    if dist == "equal":
        return torch.full((n,), 0x3F800000, dtype=torch.int32, device=device)
    if dist == "lowbyte":
        return _i32(0x5A3C1200 | ri(0, 256))
    if dist == "highbyte":
        return _i32((ri(0, 256) << 24) | 0x00ABCDEF)
    if dist == "two":
        return _i32(torch.where(rand() < 0.3, torch.full((n,), 0x00000007, device=device),
                                torch.full((n,), 0x80000003, device=device)))
    if dist in ("ascending", "descending"):
        a = torch.arange(n, dtype=torch.int64, device=device) * (2 ** 32 // max(n, 1))
        return _i32(a if dist == "ascending" else a.flip(0))
    if dist == "junk":  # ids in [lo, hi) under random bits above hi
        return _i32((ri(0, 1 << (hi - lo)) << lo) | (ri(0, 2 ** 32) & ~((1 << hi) - 1) & 0xFFFFFFFF))
    raise ValueError(dist)


@pytest.fixture
def options():
    """Sets options for one test and restores what was there before."""
    L = _lib()
    before = {}

    def set_(pairs):
        for name, value in pairs:
            before.setdefault(name, L.OPTIONS.get(name, DEFAULT_OPTIONS[name]))
            L.set_option(name, value)

    yield set_
    for name, value in before.items():
        L.set_option(name, value)


def prepare_sort(case: SortCase, keys: torch.Tensor) -> dict:
    """The buffers of one sort of `keys` (int32 [case.n]), filled on the current stream."""
    lib = _lib().load()
    cap, n = case.cap, case.n
    dev = keys.device
    bufs = [torch.full((max(cap, 1),), SENT_I32, dtype=torch.int32, device=dev) for _ in range(4)]  # k0, v0, k1, v1
    bufs[0][:n] = keys
    bufs[1][:n] = torch.arange(n, dtype=torch.int32, device=dev)
    wsb = lib.goi_raster_debug_sort_workspace_bytes(cap, case.lo, case.hi)
    assert wsb > 0
    # (not cleared by the caller: junk, so that a sort that skipped its own clear would be caught)
    ws = (torch.zeros if case.flags & 1 else lambda s, **kw: torch.full(s, 0xA5, **kw))((wsb,), dtype=torch.uint8, device=dev)
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev) if case.count is not None else None
    gh = None
    if case.ghist:
        h = digit_histograms(keys.cpu().numpy().view(np.uint32), case.lo, case.hi)
        gh = torch.from_numpy(h.view(np.int32).reshape(-1)).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    return {"bufs": bufs, "ws": ws, "n_dev": n_dev, "gh": gh, "err": err}


def call_sort(case: SortCase, b: dict, stream=None) -> int:
    """Enqueues the sort on `stream` (default: the current one); returns the index of the result buffers."""
    L = _lib()
    st = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    k0, v0, k1, v1 = (_ptr(t) for t in b["bufs"])
    r = L.load().goi_raster_debug_sort_pairs(k0, v0, k1, v1, case.cap, case.lo, case.hi, _ptr(b["n_dev"]), _ptr(b["gh"]),
                                             case.flags, _ptr(b["err"]), _ptr(b["ws"]), st)
    assert r in (0, 1), L.last_error()
    return r


def check_sorted(case: SortCase, keys: torch.Tensor, r: int, bufs, err) -> None:
    n = case.n
    assert int(err.item()) == 0, f"sort error word {int(err.item()):#x}"
    assert r == (len(pass_plan(case.lo, case.hi)) & 1 if case.cap > 0 else 0)
    host = [b.cpu().numpy().view(np.uint32) for b in bufs]
    check_sort(keys.cpu().numpy().view(np.uint32), case.lo, case.hi, host[2 * r][:n], host[2 * r + 1][:n])
    for name, b in zip(("keys0", "vals0", "keys1", "vals1"), host):
        check_untouched(name, b, n)


# ---- tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SORT_CASES, ids=lambda c: c.id)
def test_sort_matches_numpy(case, options):
    options(case.opts)
    keys = make_keys(case.dist, case.n, case.lo, case.hi, _gen(case.id))
    b = prepare_sort(case, keys)
    r = call_sort(case, b)
    torch.cuda.synchronize()
    check_sorted(case, keys, r, b["bufs"], b["err"])


def test_two_sorts_on_two_streams_at_once(options):
    """Two views in flight sort on two streams at once, each with its own workspace."""
    options(())
    cases = [S(6 * M, "depth"), S(6 * M, "tile", 0, 15)]
    keys = [make_keys(c.dist, c.n, c.lo, c.hi, _gen("streams" + c.id)) for c in cases]
    prepared = [prepare_sort(c, k) for c, k in zip(cases, keys)]
    streams = [torch.cuda.Stream() for _ in cases]
    for s in streams:  # (the inputs were written on the current stream)
        s.wait_stream(torch.cuda.current_stream())
    rs = [call_sort(c, b, s) for c, b, s in zip(cases, prepared, streams)]
    torch.cuda.synchronize()
    for c, k, r, b in zip(cases, keys, rs, prepared):
        check_sorted(c, k, r, b["bufs"], b["err"])


@pytest.mark.parametrize("case", SCAN_CASES, ids=lambda c: c.id)
def test_exclusive_scan_matches_numpy(case, options):
    options(())
    L = _lib()
    lib = L.load()
    cap, n = case.cap, case.n
    g = _gen("scan" + case.id)
    size = (max(cap, 1),)
    hi = 2 ** 32 if case.wide else 65
    vals = _i32(torch.randint(0, hi, size, generator=g, device="cuda", dtype=torch.int64))
    gather = None
    if case.gather == "perm":
        gather = torch.randperm(max(cap, 1), generator=g, device="cuda").to(torch.int32)
    elif case.gather == "repeat":
        gather = torch.randint(0, max(cap, 1), size, generator=g, device="cuda", dtype=torch.int32)
    vals_host = vals.cpu().numpy().view(np.uint32).copy()
    out = vals if case.inplace else torch.full(size, SENT_I32, dtype=torch.int32, device="cuda")
    if case.inplace:
        out[n:] = SENT_I32
    total = torch.full((1,), SENT_I32, dtype=torch.int32, device="cuda") if case.total else None
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda") if case.count is not None else None
    ws = torch.full((lib.goi_raster_debug_scan_workspace_bytes(cap),), 0xA5, dtype=torch.uint8, device="cuda")
    r = lib.goi_raster_debug_exclusive_scan(_ptr(vals), _ptr(gather), _ptr(out), cap, _ptr(n_dev), _ptr(total), _ptr(ws),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert r == 0, L.last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    g_host = None if gather is None else gather.cpu().numpy()
    check_scan(vals_host, g_host, n, got, None if total is None else int(total.cpu().numpy().view(np.uint32)[0]))
    check_untouched("out", got, n)
    if not case.inplace:
        assert np.array_equal(vals.cpu().numpy().view(np.uint32), vals_host), "the scan wrote its input"
