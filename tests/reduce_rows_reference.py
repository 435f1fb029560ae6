"""Plain numpy reference and result checkers for the backward's row reduction (csrc/reduce_rows.hip: reduce_rows_k,
find_big_k, reduce_big_k; csrc/row_sum.h: sum_instances).

Shared by tests/test_gpu_reduce_rows.py, which feeds them device results, and tests/test_reduce_rows_cpu.py, which feeds
them deliberately wrong results to show that every check can fail.

The reduction adds up one partial-gradient row per (emit-order instance, quadrant) slot, slot = instance * 4 + quadrant,
into one sum per listed Gaussian.  A Gaussian's rows are added in 16-instance chunks counted from its first instance;
inside a chunk quadrant-major (the quadrant-0 rows of the chunk's instances in instance order, then quadrant 1, ...);
only rows whose validity byte is non-zero, in fp32, from +0.  That order is replayed here exactly, so an ordinary
Gaussian's sum must match the replay BIT FOR BIT.  A BIG Gaussian (more than the frame's threshold of instances) is
split into parts and summed with compensation by reduce_big_k: it must be within BIG_ULPS * 2^-24 * sum|x| of the
float64 sum instead.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "goi_hyperplane_amd", "csrc")
U = 2.0 ** -24     # unit roundoff of fp32
BIG_ULPS = 8       # compensated sums: within BIG_ULPS * U * sum|x| of the exact sum
CHUNK = 16         # instances per chunk of sum_instances


def _src(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def kernel_constants() -> dict:
    """The reduction's thresholds and launch shapes, parsed from the sources (so that retuning one moves the tests)."""
    common, red, rs = _src("common.h"), _src("reduce_rows.hip"), _src("row_sum.h")

    def define(src, name):
        m = re.search(rf"#define {name} (\d+)\b", src)
        assert m, f"#define {name} not found"
        return int(m.group(1))

    c = {
        "BIG_INST": define(common, "GOI_REDUCE_BIG_INST"),
        "HUGE_INST": define(common, "GOI_REDUCE_HUGE_INST"),
        "DENSE_RATIO": define(common, "GOI_REDUCE_DENSE_RATIO"),
        "INFLIGHT": define(rs, "GOI_REDUCE_INFLIGHT"),
        "LARGE_SCENE": define(red, "GOI_REDUCE_LARGE_SCENE"),
        "GPQ": define(red, "GOI_REDUCE_GPQ"),
        "BIG_GRID": define(red, "GOI_REDUCE_BIG_GRID"),
    }
    m = re.search(r"constexpr int BIG_PARTS = (\d+), MID_PARTS = (\d+);", red)
    assert m, "BIG_PARTS / MID_PARTS not found"
    c["BIG_PARTS"], c["MID_PARTS"] = int(m.group(1)), int(m.group(2))
    # the frame's threshold: BIG_INST when N > DENSE_RATIO * V, SPARSE_INST otherwise -- reduce_rows_k and find_big_k alike
    sparse = re.findall(r"\(N > REDUCE_DENSE_RATIO \* \(uint32_t\)V\) \? BIG_INST : (\d+)u;", red)
    assert len(sparse) == 2 and len(set(sparse)) == 1, sparse
    c["SPARSE_INST"] = int(sparse[0])
    m = re.search(r"reduce_rows_k<K, 1, RECORD, (\d+)><<<", red)
    assert m, "the large-scene instantiation of reduce_rows_k not found"
    c["LARGE_INFLIGHT"] = int(m.group(1))
    trips = re.findall(r"if \(left <= (\d+)\) \{\s*trip\(std::integral_constant<int, (\d+)>\{\}\);", rs)
    assert len(trips) == 2 and all(a == b for a, b in trips), trips
    c["TRIPS"] = sorted(int(a) for a, _ in trips)
    m = re.search(r"inline size_t reduce_cap_big\(size_t n_cap\) \{ return \(n_cap > 0 \? n_cap : 1\) / REDUCE_BIG_INST "
                  r"\+ (\d+); \}", common)
    assert m, "reduce_cap_big not found"
    c["CAP_BIG_SPARE"] = int(m.group(1))
    return c


def cap_big(n_cap: int, c: dict) -> int:
    """Descriptor slots of a scratch laid out for n_cap instances (common.h: reduce_cap_big)."""
    return max(n_cap, 1) // c["BIG_INST"] + c["CAP_BIG_SPARE"]


def row_floats(mode: int, S: int) -> int:
    """Row width of a mode: modes 0-2 the full backward's rows, mode 3 the padded semantic channels alone."""
    nsem = 4 * ((S + 3) // 4)
    return ((nsem + 15) // 16) * 16 if mode == 3 else ((nsem + 4 + 6 + 15) // 16) * 16


# ---- frames ----------------------------------------------------------------------------------------------------------
@dataclass
class Frame:
    """What the reduction reads besides the rows: P Gaussians, V of them listed in depth order `order`, the listed one of
    rank i owning instances [offsets[i], offsets[i + 1]) (the last one up to `count`), a scratch laid out for n_cap
    instances, validity bytes [4 n_cap]."""
    P: int
    S: int
    n_cap: int
    count: int
    order: np.ndarray      # uint32 [V]
    offsets: np.ndarray    # uint32 [V]
    tiles: np.ndarray      # uint32 [P]: non-zero for the listed Gaussians
    flags: np.ndarray      # uint8 [4 n_cap]
    overflow: int = 0

    @property
    def V(self) -> int:
        return len(self.order)

    @property
    def words(self) -> np.ndarray:
        return np.array([self.count, self.V, self.overflow], dtype=np.uint32)


def make_frame(counts, P: int, S: int, rng: np.random.Generator, *, density: float = 0.4, n_cap: int | None = None,
               count: int | None = None, overflow: int = 0, flag_fn=None) -> Frame:
    """A frame whose listed Gaussians (depth ranks 0 .. len(counts) - 1) own counts[i] instances each, their ids a random
    subset of 0 .. P-1.  Validity bytes: random non-zero values at `density` (flag_fn(rank, n) -> uint8 [4 n] overrides it
    for a rank; None: keep the random ones); every slot past the ranges is flagged too (it must not be read)."""
    counts = np.asarray(counts, dtype=np.int64)
    V = len(counts)
    assert V <= P
    offsets = np.zeros(V, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)[:-1]
    total = int(counts.sum())
    n_cap = total if n_cap is None else n_cap
    count = total if count is None else count
    order = rng.permutation(P)[:V].astype(np.uint32)
    tiles = np.zeros(P, dtype=np.uint32)
    tiles[order] = np.maximum(counts, 1)  # (a listed Gaussian with no instance left: clamped by the count)
    flags = np.where(rng.random(4 * n_cap) < density, rng.integers(1, 256, 4 * n_cap), 0).astype(np.uint8)
    flags[4 * min(total, n_cap):] = rng.integers(1, 256, max(0, 4 * n_cap - 4 * total))
    if flag_fn is not None:
        for r in range(V):
            lo, hi = 4 * int(offsets[r]), 4 * int(offsets[r] + counts[r])
            if lo >= 4 * n_cap:
                break
            f = flag_fn(r, int(counts[r]))
            if f is not None:
                flags[lo:min(hi, 4 * n_cap)] = np.asarray(f, dtype=np.uint8)[:min(hi, 4 * n_cap) - lo]
    return Frame(P, S, n_cap, count, order, offsets.astype(np.uint32), tiles, flags, overflow)


def chunk_flags(n: int, per_chunk, rng: np.random.Generator) -> np.ndarray:
    """Validity bytes [4 n] of one Gaussian with per_chunk[c] (or per_chunk, an int) flagged slots in chunk c, at random
    slots of the chunk, random non-zero values."""
    f = np.zeros(4 * n, dtype=np.uint8)
    for c0 in range(0, n, CHUNK):
        k = per_chunk if np.isscalar(per_chunk) else per_chunk[c0 // CHUNK]
        slots = 4 * min(CHUNK, n - c0)
        pick = rng.choice(slots, size=min(k, slots), replace=False)
        f[4 * c0 + pick] = rng.integers(1, 256, len(pick))
    return f


# ---- the reference ---------------------------------------------------------------------------------------------------
@dataclass
class Reference:
    N: int                   # effective count
    big_inst: int
    huge_inst: int
    off0: np.ndarray         # int64 [V] clamped slot ranges (instances)
    off1: np.ndarray
    slots: np.ndarray        # int64: every row the kernel adds, in the kernel's order, rank by rank
    start: np.ndarray        # int64 [V]: a rank's first entry in slots
    length: np.ndarray       # int64 [V]: its number of rows
    big: np.ndarray = field(default=None)   # bool [V]
    huge: np.ndarray = field(default=None)  # bool [V]

    @property
    def n_inst(self) -> np.ndarray:
        return self.off1 - self.off0


def frame_reference(fr: Frame, c: dict) -> Reference:
    """Slot ranges, the frame's threshold and the rows to add in the kernel's order."""
    N = 0 if fr.overflow else min(fr.n_cap, fr.count)
    V = 0 if fr.overflow else fr.V
    off = fr.offsets.astype(np.int64)[:V]
    off0 = np.minimum(off, N)
    off1 = np.minimum(np.append(off[1:], N), N)
    n = off1 - off0
    big_inst = c["BIG_INST"] if N > c["DENSE_RATIO"] * V else c["SPARSE_INST"]
    rank = np.repeat(np.arange(V), n)
    first = np.zeros(V, dtype=np.int64)
    first[1:] = np.cumsum(n)[:-1]
    rel = np.arange(int(n.sum()), dtype=np.int64) - first[rank]   # instance relative to the Gaussian's first
    inst = off0[rank] + rel
    q = np.repeat(np.arange(4)[None, :], len(inst), 0)
    slot = inst[:, None] * 4 + q
    valid = fr.flags[slot] != 0
    r_, rel_, q_, s_ = (np.broadcast_to(a, slot.shape)[valid] for a in (rank[:, None], rel[:, None], q, slot))
    # kernel order: rank, chunk, quadrant, instance inside the chunk
    o = np.lexsort((rel_ % CHUNK, q_, rel_ // CHUNK, r_))
    slots = s_[o]
    length = np.bincount(r_, minlength=V).astype(np.int64)
    start = np.zeros(V, dtype=np.int64)
    start[1:] = np.cumsum(length)[:-1]
    ref = Reference(N, big_inst, c["HUGE_INST"], off0, off1, slots, start, length)
    ref.big = n > big_inst
    ref.huge = n > c["HUGE_INST"]
    return ref


def replay_fp32(vals: np.ndarray, start: np.ndarray, length: np.ndarray) -> np.ndarray:
    """[V, rf] float32: each rank's rows vals[start .. start + length) added one after the other in fp32 from +0."""
    vals = np.asarray(vals, dtype=np.float32)
    V = len(start)
    acc = np.zeros((V, vals.shape[1] if vals.ndim == 2 else 0), dtype=np.float32)
    if V == 0:
        return acc
    by_len = np.argsort(-length, kind="stable")
    L, st = length[by_len], start[by_len]
    a = acc[by_len]
    for j in range(int(L[0]) if V else 0):
        k = int(np.searchsorted(-L, -j, side="left"))  # ranks with more than j rows: a prefix of by_len
        a[:k] += vals[st[:k] + j]
    acc[by_len] = a
    return acc


def sums64(vals: np.ndarray, start: np.ndarray, length: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """([V, rf] float64 sums, [V, rf] float64 sums of |x|) of each rank's rows."""
    v = np.asarray(vals, dtype=np.float64)
    V, rf = len(start), v.shape[1]
    s, a = np.zeros((V, rf)), np.zeros((V, rf))
    nz = length > 0
    if nz.any():
        s[nz] = np.add.reduceat(v, start[nz], axis=0)
        a[nz] = np.add.reduceat(np.abs(v), start[nz], axis=0)
    return s, a


@dataclass
class Expected:
    """What each listed rank's sum must be: bit-equal to `plain` where not big, within `bound` of `exact` where big."""
    plain: np.ndarray   # float32 [V, rf]
    exact: np.ndarray   # float64 [V, rf]
    absum: np.ndarray   # float64 [V, rf]
    big: np.ndarray     # bool [V]
    nrows: np.ndarray   # int64 [V]

    @property
    def bound(self) -> np.ndarray:
        return BIG_ULPS * U * self.absum


def expected_sums(ref: Reference, vals: np.ndarray) -> Expected:
    """vals: [len(ref.slots), rf] the rows at ref.slots, in that order."""
    exact, absum = sums64(vals, ref.start, ref.length)
    return Expected(replay_fp32(vals, ref.start, ref.length), exact, absum, ref.big.copy(), ref.length.copy())


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def check_replay_is_sound(exp: Expected) -> None:
    """The plain replay of an ordinary Gaussian is within n_rows * U * sum|x| of float64 (the reference checks itself)."""
    ok = ~exp.big
    err = np.abs(exp.plain[ok].astype(np.float64) - exp.exact[ok])
    lim = exp.nrows[ok, None] * U * exp.absum[ok]
    assert np.all(err <= lim), "plain fp32 replay outside its own error bound"


def check_sums(got: np.ndarray, exp: Expected, ranks: np.ndarray, what: str, cols=None) -> None:
    """got: [len(ranks), rf] the kernel's sums of those listed ranks (cols: the row elements that are observable)."""
    got = np.asarray(got, dtype=np.float32)
    ranks = np.asarray(ranks, dtype=np.int64)
    cols = np.arange(got.shape[1]) if cols is None else np.asarray(cols)
    g = got[:, cols]
    if np.isnan(g).any():
        r, e = np.argwhere(np.isnan(g))[0]
        raise AssertionError(f"{what}: NaN in the sum of rank {int(ranks[r])} element {int(cols[e])}")
    big = exp.big[ranks]
    ordinary = np.flatnonzero(~big)
    want = exp.plain[ranks[ordinary]][:, cols]
    bad = _bits(g[ordinary]) != _bits(want)
    if bad.any():
        i, e = np.argwhere(bad)[0]
        r = int(ranks[ordinary[i]])
        raise AssertionError(f"{what}: rank {r} ({exp.nrows[r]} rows) element {int(cols[e])} = {g[ordinary[i], e]!r} is not "
                             f"the ordered fp32 sum {want[i, e]!r}")
    bi = np.flatnonzero(big)
    err = np.abs(g[bi].astype(np.float64) - exp.exact[ranks[bi]][:, cols])
    lim = exp.bound[ranks[bi]][:, cols]
    bad = err > lim
    if bad.any():
        i, e = np.argwhere(bad)[0]
        r = int(ranks[bi[i]])
        raise AssertionError(f"{what}: big rank {r} ({exp.nrows[r]} rows) element {int(cols[e])} = {g[bi[i], e]!r} is "
                             f"{err[i, e]:.3e} from the float64 sum {exp.exact[r, cols[e]]!r} (bound {lim[i, e]:.3e})")


# ---- the six per-id arrays (store_sums) ------------------------------------------------------------------------------
def array_widths(S: int) -> dict:
    return {"mean2D": 3, "conic": 4, "opacity": 1, "color": 3, "semantic": S, "depth": 1}


def element_map(S: int, mode: int, rf: int) -> tuple[list, dict]:
    """([rf] (array, column) or None for every row element, {array: columns written as 0}).  Modes 0-2 row layout:
    [sem 0 .. nsem) | r g b depth | mean2D x y | conic a b c | opacity | pad], nsem = 4 ceil(S / 4); channels >= S and the
    pad are dropped, mean2D z and conic [2] are written as 0, conic a b c go to [0] [1] [3].  Mode 3: semantic channels
    only."""
    nsem = 4 * ((S + 3) // 4)
    out = []
    for el in range(rf):
        if mode == 3 or el < nsem:
            out.append(("semantic", el) if el < S else None)
        elif el < nsem + 3:
            out.append(("color", el - nsem))
        elif el == nsem + 3:
            out.append(("depth", 0))
        elif el < nsem + 6:
            out.append(("mean2D", el - nsem - 4))
        elif el < nsem + 9:
            out.append(("conic", (0, 1, 3)[el - nsem - 6]))
        elif el == nsem + 9:
            out.append(("opacity", 0))
        else:
            out.append(None)
    zeros = {} if mode == 3 else {"mean2D": [2], "conic": [2]}
    return out, zeros


def arrays_to_sums(arrays: dict, ids: np.ndarray, S: int, mode: int, rf: int) -> tuple[np.ndarray, np.ndarray]:
    """([len(ids), rf] the summed rows the arrays hold for Gaussians `ids`, the observable columns)."""
    emap, _ = element_map(S, mode, rf)
    got = np.zeros((len(ids), rf), dtype=np.float32)
    cols = []
    for el, m in enumerate(emap):
        if m is not None:
            got[:, el] = arrays[m[0]].reshape(-1, array_widths(S)[m[0]])[ids, m[1]]
            cols.append(el)
    return got, np.array(cols)


def check_arrays(arrays: dict, fr: Frame, ref: Reference, exp: Expected, mode: int, rf: int) -> None:
    """Modes 0 and 3: every element of all P Gaussians written; owners (listed, at least one instance) hold their sums,
    every other Gaussian and every zero column holds +0."""
    names = ("semantic",) if mode == 3 else tuple(array_widths(fr.S))
    owners = np.flatnonzero(ref.n_inst > 0) if len(ref.n_inst) else np.zeros(0, dtype=np.int64)
    ids = fr.order[owners].astype(np.int64) if len(owners) else np.zeros(0, dtype=np.int64)
    is_owner = np.zeros(fr.P, dtype=bool)
    is_owner[ids] = True
    _, zeros = element_map(fr.S, mode, rf)
    for name in names:
        a = np.asarray(arrays[name], dtype=np.float32).reshape(fr.P, -1)
        if np.isnan(a).any():
            i, j = np.argwhere(np.isnan(a))[0]
            raise AssertionError(f"dL_d{name}[{i}][{j}] not written (or NaN)")
        b = _bits(a)
        nz = np.flatnonzero((b[~is_owner] != 0).any(1))
        if len(nz):
            i = int(np.flatnonzero(~is_owner)[nz[0]])
            raise AssertionError(f"dL_d{name}[{i}] = {a[i]} is not +0 for a Gaussian that owns no instance")
        for col in zeros.get(name, []):
            bad = np.flatnonzero(b[ids, col] != 0)
            if len(bad):
                raise AssertionError(f"dL_d{name}[{int(ids[bad[0]])}][{col}] = {a[ids[bad[0]], col]!r} must be written as +0")
    got, cols = arrays_to_sums(arrays, ids, fr.S, mode, rf)
    check_sums(got, exp, owners, "arrays", cols)


# ---- records (modes 1 and 2) -----------------------------------------------------------------------------------------
def record_ranks(ref: Reference, mode: int) -> np.ndarray:
    """Listed ranks that get a record: every one with an instance (mode 1), the big ones (mode 2)."""
    return np.flatnonzero(ref.big if mode == 2 else ref.n_inst > 0)


def record_slots(ref: Reference, ranks: np.ndarray) -> np.ndarray:
    """A record goes over the first slot its Gaussian owns (instance off0, quadrant 0)."""
    return 4 * ref.off0[ranks]


def check_only_records_written(changed: np.ndarray, allowed: np.ndarray) -> None:
    """changed: slots whose row differs in any bit after the reduction; allowed: the record slots."""
    extra = np.setdiff1d(np.asarray(changed, dtype=np.int64), np.asarray(allowed, dtype=np.int64))
    if len(extra):
        raise AssertionError(f"{len(extra)} rows outside the records were written, the first at slot {int(extra[0])}")


def big_counts(ref: Reference) -> tuple[int, int]:
    """(huge, other big) Gaussians the frame must register: big_ctl words 1 and 2."""
    return int(ref.huge.sum()), int((ref.big & ~ref.huge).sum())
