"""The backward's row reduction (csrc/reduce_rows.hip, csrc/row_sum.h) called directly, against numpy.

goi_raster_debug_reduce_rows (include/goi_raster.h) runs the product's own launchers on synthetic frames built here:
mode 0 = launch_reduce_rows into the six per-id arrays (bwd_records 0), mode 1 = its records (bwd_records 1), mode 2 =
launch_reduce_big_only (find_big_k + reduce_big_k, bwd_records 2), mode 3 = launch_reduce_sem_rows (the semantics-only
backward).  Every row the kernel must not add holds NaN: unflagged rows, rows past the count, rows no listed Gaussian
owns.  The reference (tests/reduce_rows_reference.py) replays the kernel's order in fp32, so an ordinary Gaussian's sum
must be bit-equal to it; a BIG one (reduce_big_k, compensated) must be within 8 * 2^-24 * sum|x| of the float64 sum.
Which side of the threshold a Gaussian took is observed, not assumed: a cancellation fixture whose plain fp32 sum misses
the compensated bound by 10x or more sits on both sides of every threshold.  tests/test_reduce_rows_cpu.py recomputes the
thresholds from the sources and fails when the tables here no longer straddle one.
"""
from __future__ import annotations

import ctypes as C
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from tests import reduce_rows_reference as R

pytestmark = pytest.mark.gpu

K = R.kernel_constants()
SENTINEL = float("nan")  # every output element before a call: one nobody writes is caught
BIG_GRID, BIG_INST, HUGE_INST, SPARSE_INST = K["BIG_GRID"], K["BIG_INST"], K["HUGE_INST"], K["SPARSE_INST"]
LARGE = K["LARGE_SCENE"]


# ---- helpers --------------------------------------------------------------------------------------------------------
def _lib():
    from goi_hyperplane_amd import _lib as L
    return L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _seed(tag: str) -> int:
    return zlib.crc32(tag.encode())


def make_values(n: int, rf: int, g: torch.Generator, device="cuda") -> torch.Tensor:
    """[n, rf] float32 rows: normal values, each row scaled by 2^k, k in -3 .. 3 (sums of mixed magnitudes)."""
    v = torch.randn(n, rf, generator=g, device=device, dtype=torch.float32)
    k = torch.randint(-3, 4, (n, 1), generator=g, device=device).to(torch.float32)
    return v * torch.exp2(k)


def cancellation(vals: np.ndarray, ref: R.Reference, ranks) -> np.ndarray:
    """The rows of each rank in `ranks`, in the kernel's order: +L first, -L last and small rows s in between, s of L's
    sign and below half an ulp of L: every plain fp32 addition of s to L rounds back to L, so the plain sum is 0 and the
    exact one (n - 2) s.  L = 2^(el mod 5), the sign alternating with the element."""
    vals = vals.copy()
    rf = vals.shape[1]
    el = np.arange(rf)
    L = np.exp2(el % 5).astype(np.float32) * np.where(el % 2 == 0, 1, -1).astype(np.float32)
    s = (L * np.float32(0.45 * 2.0 ** -23)).astype(np.float32)
    for r in ranks:
        a, n = int(ref.start[r]), int(ref.length[r])
        assert n >= 3
        vals[a:a + n] = s
        vals[a] = L
        vals[a + n - 1] = -L
    return vals


@dataclass
class Result:
    ref: R.Reference
    exp: R.Expected
    rf: int
    arrays: dict | None = None       # modes 0 / 3: host arrays
    records: np.ndarray | None = None  # modes 1 / 2: rows at the record slots
    rec_ranks: np.ndarray | None = None
    changed: np.ndarray | None = None  # slots whose row changed
    big_ctl: tuple | None = None


def reduce(fr: R.Frame, mode: int, tag: str, *, fixture=None, repeat=True, check=True) -> Result:
    """Builds the frame on the device, runs the reduction (twice when `repeat`: bit-identical), checks it against the
    reference (`check`) and returns what it wrote.  fixture(vals, ref) -> vals replaces the random row values."""
    L = _lib()
    lib = L.load()
    rf = lib.goi_raster_debug_reduce_row_floats(mode, fr.S)
    assert rf == R.row_floats(mode, fr.S), L.last_error()
    ref = R.frame_reference(fr, K)
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(_seed(tag))
    slots = torch.from_numpy(ref.slots).to(dev)
    vals = make_values(len(ref.slots), rf, g)
    if fixture is not None:
        vals = torch.from_numpy(fixture(vals.cpu().numpy(), ref)).to(dev)
    vals_host = vals.cpu().numpy()
    exp = R.expected_sums(ref, vals_host)
    R.check_replay_is_sound(exp)
    rows = torch.full((4 * max(fr.n_cap, 1), rf), float("nan"), dtype=torch.float32, device=dev)
    rows[slots] = vals
    del vals
    flags = torch.from_numpy(fr.flags if fr.n_cap > 0 else np.zeros(4, np.uint8)).to(dev)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)
    frame, order, offsets, tiles = i32(fr.words), i32(fr.order), i32(fr.offsets), i32(fr.tiles)
    if fr.V == 0:
        order = offsets = torch.zeros(1, dtype=torch.int32, device=dev)
    widths = R.array_widths(fr.S)
    names = ("semantic",) if mode == 3 else tuple(widths) if mode == 0 else ()
    arrays = {n: torch.empty(fr.P * widths[n], dtype=torch.float32, device=dev) for n in names}
    wsb = lib.goi_raster_debug_reduce_workspace_bytes(fr.n_cap)
    assert wsb > 0
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device=dev)  # (junk: the entry clears what must be cleared)
    before = rows.clone() if mode in (1, 2) else None
    a = lambda n: _ptr(arrays.get(n))

    def run():
        for t in arrays.values():
            t.fill_(SENTINEL)
        r = lib.goi_raster_debug_reduce_rows(mode, fr.P, fr.S, fr.n_cap, _ptr(frame), _ptr(order), _ptr(offsets), _ptr(tiles),
                                             _ptr(rows), _ptr(flags), a("mean2D"), a("conic"), a("opacity"), a("color"),
                                             a("semantic"), a("depth"), _ptr(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert r == 0, L.last_error()
        torch.cuda.synchronize()
        return ({n: t.cpu().numpy() for n, t in arrays.items()}, ws[256:288].view(torch.int32).cpu().numpy().copy())

    out, ctl = run()
    res = Result(ref, exp, rf, big_ctl=(int(ctl[1]), int(ctl[2])))
    if mode in (0, 3):
        res.arrays = out
    else:
        res.rec_ranks = R.record_ranks(ref, mode)
        rslots = torch.from_numpy(R.record_slots(ref, res.rec_ranks)).to(dev)
        res.records = rows[rslots].cpu().numpy()
        diff = (rows.view(torch.int32) != before.view(torch.int32)).any(1)
        res.changed = torch.nonzero(diff).flatten().cpu().numpy()
    if check:
        check_result(fr, mode, res)
    if repeat:  # the descriptor order differs from run to run: the sums must not
        if before is not None:
            rows.copy_(before)
        out2, ctl2 = run()
        for n in out:
            assert np.array_equal(out[n].view(np.uint32), out2[n].view(np.uint32)), f"dL_d{n}: a second run differs"
        if mode in (1, 2):
            rec2 = rows[rslots].cpu().numpy()
            assert np.array_equal(res.records.view(np.uint32), rec2.view(np.uint32)), "records: a second run differs"
        assert (int(ctl2[1]), int(ctl2[2])) == res.big_ctl
    return res


def check_result(fr: R.Frame, mode: int, res: Result) -> None:
    if mode in (0, 3):
        R.check_arrays(res.arrays, fr, res.ref, res.exp, mode, res.rf)
    else:
        R.check_only_records_written(res.changed, R.record_slots(res.ref, res.rec_ranks))
        R.check_sums(res.records, res.exp, res.rec_ranks, f"mode {mode} records")
    assert res.big_ctl == R.big_counts(res.ref), f"big Gaussians registered (huge, other) {res.big_ctl} != {R.big_counts(res.ref)}"


# ---- frames ---------------------------------------------------------------------------------------------------------
def random_counts(V: int, rng: np.random.Generator, p=0.15) -> np.ndarray:
    return rng.geometric(p, V).astype(np.int64)


def random_frame(S: int, tag: str, *, V=3001, big=(1100, 2100, 1030), P=None, **kw) -> R.Frame:
    """A few thousand listed Gaussians with geometric instance counts (mean ~7: a sparse frame), a few big ones among them;
    V not a multiple of 16 or 32, P well above V."""
    rng = np.random.default_rng(_seed(tag))
    counts = random_counts(V, rng)
    counts[rng.choice(V, len(big), replace=False)] = big
    return R.make_frame(counts, P or 3 * V + 7, S, rng, **kw)


def walk_counts():
    """(instances, flagged rows per chunk or None for random) of every rank, in waves of four consecutive ranks (the four
    quarter waves of one wave: the loop runs to the wave's largest count)."""
    w = [
        [(0, None), (1, None), (15, None), (16, None)],
        [(17, None), (63, None), (64, None), (65, None)],
        [(129, None), (1, 4), (0, None), (129, 64)],
        [(65, [3, 0, 4, 0, 1])] * 4,                      # chunks 1 and 3 empty in every quarter: skipped on one ballot
        [(33, [0, 0, 2]), (16, 0), (40, [0, 0, 0]), (1, 0)],
    ]
    for k in (4, 5, 12, 13, 16, 17, 32, 33, 64):         # trip boundaries: 4 / 12 / 16 or 32 rows in flight
        w.append([(32, [k, k]), (16, [k]), (48, [1, k, 0]), (17, [max(k - 1, 0), 1])])
        w.append([(16, [k])] * 4)
    return [x for wave in w for x in wave]


def walk_frame(S: int, P: int, tag: str) -> R.Frame:
    rng = np.random.default_rng(_seed(tag))
    spec = walk_counts() * 2
    spec += [(int(c), None) for c in random_counts(37, rng)]  # (V not a multiple of 16)
    counts = [n for n, _ in spec]

    def flag_fn(r, n):
        k = spec[r][1]
        return None if k is None else R.chunk_flags(n, k, rng)
    return R.make_frame(counts, P, S, rng, density=0.5, flag_fn=flag_fn)


FIXTURE_COUNTS = (BIG_INST, BIG_INST + 1, SPARSE_INST, SPARSE_INST + 1, HUGE_INST, HUGE_INST + 1)


def threshold_frame(kind: str, S: int) -> tuple[R.Frame, np.ndarray]:
    """(frame, ranks of the fixture Gaussians) with the cancellation fixture at every threshold count.  dense: N > 10 V;
    sparse_eq: N == 10 V exactly; sparse_lt: N < 10 V."""
    rng = np.random.default_rng(_seed("threshold" + kind))
    fix = list(FIXTURE_COUNTS)
    ratio = K["DENSE_RATIO"]
    if kind == "dense":
        fill = list(random_counts(300, rng, 0.25))
    else:
        d = sum(fix) - ratio * len(fix)   # each filler of c instances changes N - ratio V by c - ratio
        q, r = divmod(d, ratio - 1)
        fill = [1] * q + ([ratio - r] if r else []) + ([1] if kind == "sparse_lt" else [])
    counts = np.array(fix + fill, dtype=np.int64)
    perm = rng.permutation(len(counts))
    counts = counts[perm]
    fixture_ranks = np.flatnonzero(perm < len(fix))
    N, V = int(counts.sum()), len(counts)
    assert (N > ratio * V) == (kind == "dense") and (N == ratio * V) == (kind == "sparse_eq")
    full = lambda r, n: rng.integers(1, 256, 4 * n) if r in set(fixture_ranks.tolist()) else None
    return R.make_frame(counts, 2 * V + 3, S, rng, density=0.4, flag_fn=full), fixture_ranks


# ---- 1. every row width and mode ------------------------------------------------------------------------------------
# every semantic width the rasterizer admits (the 16-byte output path of S % 4 == 0 and the scalar one at every row width;
# tests/test_channel_counts_cpu.py counts the classes); mode 2 exists for the 128-byte rows only (S = 5 .. 20)
WIDTH_CASES = ([(0, S) for S in range(1, 33)] + [(1, S) for S in range(1, 33)] + [(3, S) for S in range(1, 33)]
               + [(2, S) for S in range(5, 21)])


@pytest.mark.parametrize("mode,S", WIDTH_CASES, ids=lambda x: str(x))
def test_random_frame_every_width(mode, S):
    fr = random_frame(S, f"width{mode}-{S}")
    res = reduce(fr, mode, f"width{mode}-{S}")
    assert res.ref.big.sum() == 3 and res.ref.huge.sum() == 1


# ---- 2. walk shapes, at both in-flight settings ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 3])
@pytest.mark.parametrize("P", [5000, LARGE], ids=["P5000", "P_large"])
def test_walk_shapes(mode, P):
    fr = walk_frame(8, P, f"walk{P}")
    reduce(fr, mode, f"walk{mode}-{P}", repeat=P < LARGE)


# ---- 3. the BIG thresholds, observed through the cancellation fixture -------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["dense", "sparse_eq", "sparse_lt"])
def test_big_threshold(kind, mode):
    fr, fix = threshold_frame(kind, 8)
    res = reduce(fr, mode, f"thr{kind}", fixture=lambda v, ref: cancellation(v, ref, fix))
    ref, exp = res.ref, res.exp
    # premise: the plain fp32 sum of every fixture Gaussian misses the compensated bound by 10x or more
    miss = np.abs(exp.plain[fix].astype(np.float64) - exp.exact[fix]) / exp.bound[fix]
    assert miss.min() >= 10, miss.min()
    n = ref.n_inst[fix]
    thr = BIG_INST if kind == "dense" else SPARSE_INST
    assert ref.big_inst == thr
    assert set(n[ref.big[fix]].tolist()) == {c for c in FIXTURE_COUNTS if c > thr}  # (what check_result observed)


# ---- 4. persistent-grid trips and a descriptor list packed to cap_big -----------------------------------------------
def persistent_counts(rng: np.random.Generator) -> np.ndarray:
    counts = [BIG_INST + 1] * (4 * BIG_GRID + 5) + [HUGE_INST + 1] * (BIG_GRID + 3) + list(random_counts(203, rng))
    return np.array(counts)[rng.permutation(len(counts))]


def test_persistent_grid_trips():
    """More than 4 BIG_GRID mid-size big Gaussians and more than BIG_GRID huge ones: every workgroup of reduce_big_k
    takes several descriptors of each kind (64-byte rows)."""
    rng = np.random.default_rng(_seed("persistent"))
    counts = persistent_counts(rng)
    fr = R.make_frame(counts, len(counts) + 1000, 4, rng, density=0.25)
    res = reduce(fr, 0, "persistent", repeat=False)
    assert res.big_ctl == (BIG_GRID + 3, 4 * BIG_GRID + 5)


def test_descriptor_list_packed_to_cap_big():
    """Every Gaussian has BIG_INST + 1 instances and the scratch holds exactly their instances: the list is filled from its
    end to within a few entries of its front."""
    rng = np.random.default_rng(_seed("packed"))
    G = 4 * BIG_GRID + 52
    fr = R.make_frame([BIG_INST + 1] * G, G + 17, 1, rng, density=0.3)
    cap = R.cap_big(fr.n_cap, K)
    assert G <= cap <= G + G // BIG_INST + K["CAP_BIG_SPARE"]
    res = reduce(fr, 1, "packed")
    assert res.big_ctl == (0, G)


# ---- 5. frame states ------------------------------------------------------------------------------------------------
def _state_frame(state: str) -> R.Frame:
    rng = np.random.default_rng(_seed("state" + state))
    counts = random_counts(1501, rng)
    counts[[100, 700, 1200]] = (1100, 2100, 40)
    total = int(counts.sum())
    offs = np.concatenate([[0], np.cumsum(counts)])
    if state == "overflow":
        return R.make_frame(counts, 4000, 8, rng, overflow=1)
    if state == "below_cap":   # slots past the count are flagged and hold NaN
        return R.make_frame(counts, 4000, 8, rng, n_cap=total + 777)
    if state == "above_cap":   # a speculative frame that overflowed: the scratch holds the first n_cap instances
        return R.make_frame(counts, 4000, 8, rng, n_cap=int(offs[1200]) + 17)
    if state == "above_cap_big":  # the cut leaves 500 of a big Gaussian's instances: it is summed as an ordinary one
        return R.make_frame(counts, 4000, 8, rng, n_cap=int(offs[100]) + 500)
    if state == "count0":
        return R.make_frame(counts, 4000, 8, rng, count=0)
    raise ValueError(state)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("state", ["overflow", "below_cap", "above_cap", "above_cap_big", "count0"])
def test_frame_states(state, mode):
    fr = _state_frame(state)
    res = reduce(fr, mode, f"state{state}")
    if state in ("overflow", "count0"):
        assert res.ref.N == 0 and (res.changed is None or len(res.changed) == 0)
    if state.startswith("above_cap"):
        straddle = 1200 if state == "above_cap" else 100
        assert 0 < res.ref.n_inst[straddle] < fr.offsets[straddle + 1] - fr.offsets[straddle]
        assert np.all(res.ref.n_inst[straddle + 1:] == 0)
        assert not res.ref.big[straddle]


# ---- 6. the large-scene switch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_large_scene_switch_is_bit_identical(mode):
    """The same listed Gaussians at P = LARGE_SCENE - 1 (GPQ Gaussians per quarter wave, INFLIGHT rows in flight) and
    P = LARGE_SCENE (one Gaussian, 16 rows): the same sums, bit for bit, both the replay's."""
    a = walk_frame(8, LARGE - 1, "switch")
    b = R.Frame(LARGE, a.S, a.n_cap, a.count, a.order, a.offsets, np.append(a.tiles, np.uint32(0)), a.flags)
    ra = reduce(a, mode, "switch", repeat=False)
    rb = reduce(b, mode, "switch", repeat=False)
    if mode == 0:
        for n in ra.arrays:
            w = R.array_widths(a.S)[n]
            assert np.array_equal(ra.arrays[n].view(np.uint32), rb.arrays[n][:(LARGE - 1) * w].view(np.uint32)), n
    else:
        assert np.array_equal(ra.records.view(np.uint32), rb.records.view(np.uint32))


# ---- 7. the modes agree ---------------------------------------------------------------------------------------------
def test_modes_agree():
    fr = random_frame(8, "agree", big=(400, 1100, 2100, 3000, 1025))
    r0, r1, r2 = (reduce(fr, m, "agree", repeat=False) for m in (0, 1, 2))
    ids = fr.order[r1.rec_ranks].astype(np.int64)
    sums0, cols = R.arrays_to_sums(r0.arrays, ids, fr.S, 0, r0.rf)
    assert np.array_equal(sums0[:, cols].view(np.uint32), r1.records[:, cols].view(np.uint32)), "mode 1 records != mode 0 arrays"
    pos = {int(r): i for i, r in enumerate(r1.rec_ranks)}
    big1 = r1.records[[pos[int(r)] for r in r2.rec_ranks]]
    assert len(r2.rec_ranks) == int(r1.ref.big.sum()) >= 4
    assert np.array_equal(big1.view(np.uint32), r2.records.view(np.uint32)), "mode 2 records != mode 1 records"
