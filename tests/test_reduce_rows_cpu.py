"""CPU checks that keep tests/test_gpu_reduce_rows.py honest (no GPU needed):
  * the constants it straddles parse out of the kernel sources, and its case tables straddle every threshold derived
    from them -- retuning one fails here instead of silently losing coverage;
  * its checkers fail on each kind of subtly wrong sum a broken reduction would produce;
  * the entry point refuses bad arguments before any HIP call.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import reduce_rows_reference as R
from tests import test_gpu_reduce_rows as G

K = R.kernel_constants()


# ---- constants and tables -------------------------------------------------------------------------------------------
def test_kernel_constants_parse():
    c = K
    assert 0 < c["BIG_INST"] < c["SPARSE_INST"] < c["HUGE_INST"]
    assert c["DENSE_RATIO"] > 1 and c["GPQ"] >= 1 and c["BIG_GRID"] >= 1
    assert c["MID_PARTS"] < c["BIG_PARTS"] and c["BIG_PARTS"] * 16 == 1024  # (a 1024-thread workgroup of quarter waves)
    assert c["LARGE_INFLIGHT"] < c["INFLIGHT"] and c["TRIPS"] == sorted(c["TRIPS"]) and c["TRIPS"][-1] < c["LARGE_INFLIGHT"]
    assert c["LARGE_SCENE"] > 0 and c["CAP_BIG_SPARE"] >= 1
    # the scratch layout (api.hip) and the test entry (reduce_rows.hip) both take cap_big from the one helper
    api, unit = R._src("api.hip"), R._src("reduce_rows.hip")
    assert api.count("reduce_cap_big(") == 1 and unit.count("reduce_cap_big(") == 1
    assert "/ REDUCE_BIG_INST" not in api and "/ REDUCE_BIG_INST" not in unit


def _parts_used(n, parts):
    per = ((n + parts - 1) // parts + 63) & ~63
    return -(-n // per)


def test_threshold_fixtures_straddle_every_threshold():
    c = K
    fix = set(G.FIXTURE_COUNTS)
    for t in (c["BIG_INST"], c["SPARSE_INST"], c["HUGE_INST"]):
        assert {t, t + 1} <= fix
    # part splits that leave empty trailing parts, in both part counts
    assert any(_parts_used(n, c["BIG_PARTS"]) < c["BIG_PARTS"] for n in fix if n > c["HUGE_INST"])
    assert any(_parts_used(n, c["MID_PARTS"]) < c["MID_PARTS"] for n in fix if c["BIG_INST"] < n <= c["HUGE_INST"])
    for kind in ("dense", "sparse_eq", "sparse_lt"):
        fr, ranks = G.threshold_frame(kind, 8)
        N, V = fr.count, fr.V
        assert {"dense": N > c["DENSE_RATIO"] * V, "sparse_eq": N == c["DENSE_RATIO"] * V,
                "sparse_lt": N < c["DENSE_RATIO"] * V}[kind]
        n = np.diff(np.append(fr.offsets.astype(np.int64), N))
        assert sorted(n[ranks].tolist()) == sorted(G.FIXTURE_COUNTS)
        assert np.all(fr.flags[np.concatenate([np.arange(4 * fr.offsets[r], 4 * (fr.offsets[r] + n[r])) for r in ranks])])


def test_walk_table_straddles_every_trip():
    spec = G.walk_counts()
    counts = {n for n, _ in spec}
    assert {0, 1, 15, 16, 17, 63, 64, 65, 129} <= counts
    per_chunk = set()
    for n, k in spec:
        if k is not None:
            per_chunk |= {k} if np.isscalar(k) else set(k)
    for t in K["TRIPS"] + [K["INFLIGHT"], K["LARGE_INFLIGHT"]]:
        assert {t, t + 1} <= per_chunk, t
    assert 64 in per_chunk and 0 in per_chunk
    assert len(spec) % 4 == 0  # (waves of four quarter waves)
    waves = [spec[i:i + 4] for i in range(0, len(spec), 4)]
    assert any(max(n for n, _ in w) > 8 * max(min(n for n, _ in w), 1) for w in waves)  # very different counts in one wave
    assert any(all(k is not None and not np.isscalar(k) and len(k) > 1 and k[1] == 0 for _, k in w) for w in waves)  # ballot skip
    fr = G.walk_frame(8, 5000, "walk5000")
    assert fr.V % 16 and fr.V % 32 and fr.P > fr.V


def test_width_and_scale_tables():
    rf = {(m, R.row_floats(m, S)) for m, S in G.WIDTH_CASES}
    assert {(0, 16), (0, 32), (0, 48), (1, 16), (1, 32), (1, 48), (3, 16), (3, 32), (2, 32)} <= rf
    assert all(R.row_floats(2, S) == 32 for m, S in G.WIDTH_CASES if m == 2)
    rng = np.random.default_rng(1)
    counts = G.persistent_counts(rng)
    assert (counts == K["BIG_INST"] + 1).sum() > 4 * K["BIG_GRID"] and (counts > K["HUGE_INST"]).sum() > K["BIG_GRID"]
    fr = G.random_frame(4, "width0-4")
    assert fr.V % 16 and fr.V % 32 and fr.P > 2 * fr.V
    assert fr.count <= K["DENSE_RATIO"] * fr.V  # (sparse: the three big ones are registered at SPARSE_INST)


# ---- the checkers are sensitive --------------------------------------------------------------------------------------
def _setup(S=8, mode=0, fixture_ranks=None, frame=None, tag="cpu"):
    fr = frame or G.walk_frame(S, 700, tag)
    ref = R.frame_reference(fr, K)
    rf = R.row_floats(mode, S)
    g = torch.Generator().manual_seed(5)
    vals = G.make_values(len(ref.slots), rf, g, device="cpu").numpy()
    if fixture_ranks is not None:
        vals = G.cancellation(vals, ref, fixture_ranks)
    return fr, ref, rf, vals, R.expected_sums(ref, vals)


def _arrays(fr, ref, exp, mode, rf, sums=None):
    """The arrays a correct kernel writes: sums (default: the plain replay, the float64 sum for big ranks) of the owners
    through the element map, +0 everywhere else."""
    if sums is None:
        sums = np.where(exp.big[:, None], exp.exact.astype(np.float32), exp.plain)
    widths = R.array_widths(fr.S)
    names = ("semantic",) if mode == 3 else tuple(widths)
    out = {n: np.zeros((fr.P, widths[n]), dtype=np.float32) for n in names}
    emap, _ = R.element_map(fr.S, mode, rf)
    owners = np.flatnonzero(ref.n_inst > 0)
    for el, m in enumerate(emap):
        if m is not None:
            out[m[0]][fr.order[owners], m[1]] = sums[owners, el]
    return {n: a.reshape(-1) for n, a in out.items()}


def test_checkers_accept_the_reference():
    for mode in (0, 3):
        fr, ref, rf, vals, exp = _setup(mode=mode)
        R.check_replay_is_sound(exp)
        R.check_arrays(_arrays(fr, ref, exp, mode, rf), fr, ref, exp, mode, rf)
    ranks = R.record_ranks(ref, 1)
    R.check_sums(exp.plain[ranks], exp, ranks, "records")
    R.check_only_records_written(R.record_slots(ref, ranks)[::3], R.record_slots(ref, ranks))


def _ranks_with(ref, rows):
    return np.flatnonzero(ref.length >= rows)


def test_check_sums_rejects_a_dropped_and_a_doubled_row():
    fr, ref, rf, vals, exp = _setup()
    r = int(_ranks_with(ref, 3)[0])
    a, n = int(ref.start[r]), int(ref.length[r])
    for wrong in (np.delete(vals, a + 1, 0), np.insert(vals, a + 1, vals[a + 1], 0)):
        length = ref.length.copy()
        length[r] += len(wrong) - len(vals)
        start = np.zeros_like(length)
        start[1:] = np.cumsum(length)[:-1]
        got = R.replay_fp32(wrong, start, length)
        with pytest.raises(AssertionError, match=f"rank {r} "):
            R.check_sums(got[r:r + 1], exp, np.array([r]), "records")


def test_check_sums_rejects_slot_order():
    """Instance-major ("slot order") sums differ in bits from the kernel's quadrant-major ones on this frame."""
    fr, ref, rf, vals, exp = _setup()
    by_slot = np.concatenate([np.argsort(ref.slots[a:a + n], kind="stable") + a for a, n in zip(ref.start, ref.length)])
    got = R.replay_fp32(vals[by_slot], ref.start, ref.length)
    differ = np.flatnonzero((got.view(np.uint32) != exp.plain.view(np.uint32)).any(1))
    assert len(differ) > 10  # (premise: the two orders are told apart)
    with pytest.raises(AssertionError, match="ordered fp32 sum"):
        R.check_sums(got, exp, np.arange(len(got)), "records")
    # and through the arrays
    with pytest.raises(AssertionError, match="ordered fp32 sum"):
        R.check_arrays(_arrays(fr, ref, exp, 0, rf, got), fr, ref, exp, 0, rf)


def test_check_arrays_rejects_mapping_mistakes():
    fr, ref, rf, vals, exp = _setup(S=5)
    good = _arrays(fr, ref, exp, 0, rf)
    owner = int(fr.order[np.flatnonzero(ref.length > 0)[0]])
    cases = []
    a = {n: v.copy() for n, v in good.items()}
    c = a["conic"].reshape(-1, 4)
    c[:, [0, 1]] = c[:, [1, 0]]  # conic a, b swapped
    cases.append((a, "ordered fp32 sum"))
    a = {n: v.copy() for n, v in good.items()}
    a["conic"].reshape(-1, 4)[owner, 2] = 1.0
    cases.append((a, r"conic\[%d\]\[2\]" % owner))
    a = {n: v.copy() for n, v in good.items()}
    a["mean2D"].reshape(-1, 3)[owner, 2] = -0.0  # (a -0 is not the +0 written)
    cases.append((a, r"mean2D\[%d\]\[2\]" % owner))
    a = {n: v.copy() for n, v in good.items()}
    a["color"].reshape(-1, 3)[owner] = a["color"].reshape(-1, 3)[owner, ::-1]
    cases.append((a, "ordered fp32 sum"))
    a = {n: v.copy() for n, v in good.items()}
    a["opacity"][owner], a["depth"][owner] = a["depth"][owner], a["opacity"][owner]
    cases.append((a, "ordered fp32 sum"))
    a = {n: v.copy() for n, v in good.items()}
    a["semantic"].reshape(-1, 5)[owner, 4] = np.nan  # an element nobody wrote
    cases.append((a, "not written"))
    a = {n: v.copy() for n, v in good.items()}
    other = int(np.setdiff1d(np.arange(fr.P), fr.order[ref.n_inst > 0])[0])
    a["depth"][other] = 1e-30  # a Gaussian without rows that is not zeroed
    cases.append((a, "owns no instance"))
    for arrays, msg in cases:
        with pytest.raises(AssertionError, match=msg):
            R.check_arrays(arrays, fr, ref, exp, 0, rf)


def test_check_only_records_written_rejects_another_row():
    fr, ref, rf, vals, exp = _setup()
    rec = R.record_slots(ref, R.record_ranks(ref, 1))
    with pytest.raises(AssertionError, match="outside the records"):
        R.check_only_records_written(np.append(rec, rec[0] + 1), rec)


def test_check_sums_rejects_a_big_gaussian_summed_plainly():
    """The cancellation fixture: the plain sum of a big Gaussian misses the compensated bound."""
    counts = np.full(40, 3)
    counts[[5, 20]] = (K["SPARSE_INST"] + 1, K["HUGE_INST"] + 1)
    fr = R.make_frame(counts, 100, 8, np.random.default_rng(2), flag_fn=lambda r, n: np.ones(4 * n) if n > 3 else None)
    ref = R.frame_reference(fr, K)
    fr_, ref, rf, vals, exp = _setup(frame=fr, fixture_ranks=[5, 20])
    assert exp.big[[5, 20]].all()
    R.check_sums(exp.exact[[5, 20]].astype(np.float32), exp, np.array([5, 20]), "records")
    with pytest.raises(AssertionError, match="big rank 5 .* from the float64 sum"):
        R.check_sums(exp.plain[[5, 20]], exp, np.array([5, 20]), "records")
    # and an ordinary Gaussian summed with compensation is not the plain replay
    exp.big[5] = False
    with pytest.raises(AssertionError, match="rank 5 .* ordered fp32 sum"):
        R.check_sums(exp.exact[[5]].astype(np.float32), exp, np.array([5]), "records")


def test_reference_frame_rules():
    """Clamping to min(n_cap, count), a set overflow word, the dense / sparse rule and the kernel's order."""
    counts = np.array([3, 0, 20, 5])
    fr = R.make_frame(counts, 10, 4, np.random.default_rng(0), density=1.0, n_cap=25)
    ref = R.frame_reference(fr, K)
    assert ref.N == 25 and ref.n_inst.tolist() == [3, 0, 20, 2]
    s = ref.slots[ref.start[2]:ref.start[2] + ref.length[2]] - 4 * 3
    want = [4 * i + q for c0 in (0, 16) for q in range(4) for i in range(c0, min(c0 + 16, 20))]
    assert s.tolist() == want  # chunks of 16, quadrant-major inside
    fr.overflow = 1
    assert R.frame_reference(fr, K).N == 0 and len(R.frame_reference(fr, K).slots) == 0
    fr.overflow, fr.count = 0, 0
    assert R.frame_reference(fr, K).n_inst.tolist() == [0, 0, 0, 0]
    r = K["DENSE_RATIO"]
    for N, want_thr in ((r * 4 + 1, K["BIG_INST"]), (r * 4, K["SPARSE_INST"])):
        f = R.make_frame([N - 3, 1, 1, 1], 4, 4, np.random.default_rng(0))
        assert R.frame_reference(f, K).big_inst == want_thr
    assert R.cap_big(0, K) == R.cap_big(1, K) == K["CAP_BIG_SPARE"] and R.cap_big(K["BIG_INST"] * 7, K) == 7 + K["CAP_BIG_SPARE"]


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
MISALIGNED = C.c_void_p((1 << 20) + 64)


def _call(lib, mode, P=100, S=8, n_cap=1000, null=(), ws=MISALIGNED):
    names = ("frame", "order", "offsets", "tiles", "rows", "flags", "mean2D", "conic", "opacity", "color", "semantic", "depth")
    ptrs = [None if n in null else FAKE for n in names]
    return lib.goi_raster_debug_reduce_rows(mode, P, S, n_cap, *ptrs, None if "ws" in null else ws, None)


def test_row_floats(lib):
    for S in range(1, 33):
        for mode in (0, 1):
            assert lib.goi_raster_debug_reduce_row_floats(mode, S) == R.row_floats(mode, S)
        assert lib.goi_raster_debug_reduce_row_floats(3, S) == R.row_floats(3, S)
        want2 = 32 if R.row_floats(2, S) == 32 else -1
        assert (lib.goi_raster_debug_reduce_row_floats(2, S) == 32) == (want2 == 32)
        if want2 < 0:
            assert lib.goi_raster_debug_reduce_row_floats(2, S) < 0 and "128-byte" in _err(lib)
    for mode, S in ((-1, 8), (4, 8), (0, 0), (0, 33), (3, 0)):
        assert lib.goi_raster_debug_reduce_row_floats(mode, S) < 0


def test_workspace_bytes(lib):
    assert lib.goi_raster_debug_reduce_workspace_bytes(-1) == 0
    assert lib.goi_raster_debug_reduce_workspace_bytes(1 << 31) == 0
    w0, w1 = lib.goi_raster_debug_reduce_workspace_bytes(0), lib.goi_raster_debug_reduce_workspace_bytes(10_000_000)
    assert w0 >= 512 + 16 * R.cap_big(0, K)
    assert w1 >= 512 + 16 * R.cap_big(10_000_000, K) and w1 > w0


@pytest.mark.parametrize("mode,S,msg", [(-1, 8, "unknown mode"), (4, 8, "unknown mode"), (0, 0, "1 <= S <= 32"),
                                        (1, 33, "1 <= S <= 32"), (2, 4, "128-byte"), (2, 21, "128-byte")])
def test_refuses_bad_mode_and_width(lib, mode, S, msg):
    assert _call(lib, mode, S=S) < 0
    assert msg in _err(lib)


def test_refuses_bad_sizes(lib):
    for P, n_cap in ((-1, 10), (10, -1), (10, 1 << 31)):
        assert _call(lib, 0, P=P, n_cap=n_cap) < 0 and "n_cap" in _err(lib)
    assert _call(lib, 0, P=0, null=("frame", "rows", "ws")) == 0  # (nothing to do)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_refuses_null_pointers(lib, mode):
    required = {"frame", "order", "offsets", "rows", "flags", "ws"}
    if mode in (0, 3):
        required |= {"tiles", "semantic"}
    if mode == 0:
        required |= {"mean2D", "conic", "opacity", "color", "depth"}
    for name in sorted(required):
        assert _call(lib, mode, null=(name,)) < 0, name
        assert "NULL" in _err(lib), name
    # every pointer the mode does not read may be NULL: such a call gets as far as the alignment check
    optional = {"tiles", "mean2D", "conic", "opacity", "color", "semantic", "depth"} - required
    assert _call(lib, mode, null=tuple(optional)) < 0 and "256-byte aligned" in _err(lib)
