"""The semantic head's kernels called directly through the C ABI, against tests/semantic_head_reference.py.

goi_semantic_decode: every instantiation (semantic_decode3n_k<2, 4, 1> under decode_variant 1, 2, 3;
semantic_decode_k<K4, 0> for K4 = 1 .. 8 and <4, 19>), checked pixel by pixel with the eps-argmax rule (no agreement
rates), at shapes that straddle the 16-pixel block, the 16 NPB-pixel unit, the 64-pixel group, the fp32 kernel's
persistent trip (GRID_CAP workgroups x 256 pixels), 16-code blocks and both LDS bounds; on fixtures that make a subtle
error visible (near-tie ladder, exact ties, zero features, all-negative logits, mixed magnitudes, thresholds).
goi_codebook_loss_rows: every codes-per-lane instantiation at its edges, element by element against float64.
Every output starts as a sentinel (NaN / 0xAB) with one extra tail element; tests/test_semantic_head_cpu.py checks
that the tables here straddle the bounds parsed from the sources.
"""
from __future__ import annotations

import ctypes as C
import zlib

import pytest
import torch

from tests import semantic_head_reference as R

pytestmark = pytest.mark.gpu

K = R.kernel_constants()
IDX_SENTINEL = int.from_bytes(b"\xab" * 4, "little", signed=True)
BG_SENTINEL = 0xAB
WORST = {}  # largest error seen as a fraction of its bound, per path / output (printed at the end of the module)


def _lib():
    from goi_hyperplane_amd import _lib as L
    return L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _seed(tag) -> int:
    return zlib.crc32(repr(tag).encode())


def _note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), value)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"worst error / bound {k}: {WORST[k]:.4f}")


# ---- decode ---------------------------------------------------------------------------------------------------------
# (decode_variant, S): the split kernel with 2, 4, 1 pixel blocks per fetch, the fp32 kernel at K4 = 1 .. 8
PATHS = ([(1, S) for S in (1, 2, 7, 8, 9, 16)] + [(2, S) for S in (1, 8, 16)] + [(3, S) for S in (1, 9, 16)]
         + [(0, S) for S in (1, 4, 5, 8, 11, 13, 16)] + [(1, S) for S in (17, 20, 23, 25, 29, 32)])
HW_EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
CODE_EDGES = (1, 15, 16, 17, 300, 301)
TRIP = K["GRID_CAP"] * 256
SPLIT_MAX = R.split_max_codes(K)


def decode(sem, W, b, n_codes, variant, code_score=None, thresh=0.5, outputs=("sim", "idx", "bg")):
    """One goi_semantic_decode call on sentinel-filled outputs with a tail element; returns (rc, sim, idx, bg)."""
    L = _lib()
    S, HW = sem.shape
    dev = sem.device
    sim = torch.full((HW + 1,), float("nan"), device=dev) if "sim" in outputs else None
    idx = torch.full((HW + 1,), IDX_SENTINEL, dtype=torch.int32, device=dev) if "idx" in outputs else None
    bg = torch.full((HW + 1,), BG_SENTINEL, dtype=torch.uint8, device=dev) if "bg" in outputs else None
    L.set_option("decode_variant", variant)
    try:
        rc = L.load().goi_semantic_decode(_ptr(sem), S, HW, _ptr(W), _ptr(b), n_codes, _ptr(code_score), float(thresh),
                                          _ptr(sim), _ptr(idx), _ptr(bg), None)
        torch.cuda.synchronize()
    finally:
        L.set_option("decode_variant", 1)
    for t, s in ((sim, None), (idx, IDX_SENTINEL), (bg, BG_SENTINEL)):
        if t is not None:
            tail = t[HW:]
            assert (torch.isnan(tail).all() if s is None else (tail == s).all()), "write past the end"
    return rc, (sim[:HW] if sim is not None else None), (idx[:HW] if idx is not None else None), \
        (bg[:HW] if bg is not None else None)


def scores(n_codes, dev, seed):
    """code_score with 16 spare elements behind it (a padding index could never read outside the allocation)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(n_codes + 16, generator=g)).to(dev)[:n_codes]


def check_decode(sem, W, b, n_codes, variant, score, thresh=0.5):
    S = sem.shape[0]
    path = R.decode_path(S, n_codes, variant, K)
    rc, sim, idx, bg = decode(sem, W, b, n_codes, variant, score, thresh)
    assert rc == 0, _lib().last_error()
    assert (idx != IDX_SENTINEL).all() and (bg != BG_SENTINEL).all() and not torch.isnan(sim).any(), "pixel not written"
    worst = R.decode_check(sem, W, b, idx, R.gamma(path, S))
    _note(f"decode {path}", worst)
    R.decode_outputs_check(idx, score, thresh, sim, bg)
    return idx, sim, bg


def random_problem(S, HW, n_codes, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    sem = torch.randn(S, HW, generator=g).to(dev)
    W = torch.randn(n_codes, S, generator=g).to(dev)
    b = torch.randn(n_codes, generator=g).to(dev) * 0.5
    return sem, W, b


@pytest.mark.parametrize("variant,S", PATHS)
def test_decode_shapes(variant, S):
    """Every HW edge x every code-count edge; the split kernel's NPB = 1, 2, 4 must agree bit for bit."""
    dev = torch.device("cuda")
    for HW in HW_EDGES + (1000,):
        for n in CODE_EDGES:
            sem, W, b = random_problem(S, HW, n, _seed((S, HW, n)), dev)
            score = scores(n, dev, _seed((n, "s")))
            idx, sim, bg = check_decode(sem, W, b, n, variant, score)
            if variant >= 1 and S <= 16:
                for v in (1, 2, 3):
                    _, sim_v, idx_v, bg_v = decode(sem, W, b, n, v, score)
                    assert torch.equal(idx_v, idx) and torch.equal(sim_v.view(torch.int32), sim.view(torch.int32)) \
                        and torch.equal(bg_v, bg), (v, HW, n)


def test_decode_fixed_block_specialisation():
    """semantic_decode_k<4, 19>: 289 .. 304 codes at S = 13 .. 16 under decode_variant 0."""
    dev = torch.device("cuda")
    for S, n in ((16, 300), (13, 289), (16, 304), (14, 297)):
        assert R.decode_path(S, n, 0, K) == ("fp32", K["FIXED_K4"], K["FIXED_NBLK"])
        for HW in (1, 65, 5000):
            sem, W, b = random_problem(S, HW, n, _seed((S, n, HW, "fixed")), dev)
            check_decode(sem, W, b, n, 0, scores(n, dev, 1))


@pytest.mark.parametrize("S,variant", [(16, 0), (32, 1), (3, 0)])
def test_decode_fp32_persistent_trip(S, variant):
    """HW around GRID_CAP workgroups x 256 pixels: the last pixels of one trip and the first of the next."""
    dev = torch.device("cuda")
    for HW in (TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 77):
        sem, W, b = random_problem(S, HW, 37, _seed((S, HW, "trip")), dev)
        check_decode(sem, W, b, 37, variant, scores(37, dev, 2))


def test_decode_split_multi_trip_and_npb_agreement():
    """About 1 M pixels (more units than resident workgroups: several trips of the persistent grid), 300 and 301
    codes (odd and even block counts); NPB = 1, 2, 4 bit-identical."""
    dev = torch.device("cuda")
    HW = (1 << 20) + 17
    for n in (300, 288, 301):
        sem, W, b = random_problem(16, HW, n, _seed((n, "big")), dev)
        score = scores(n, dev, 3)
        idx, sim, bg = check_decode(sem, W, b, n, 1, score)
        for v in (2, 3):
            _, sim_v, idx_v, bg_v = decode(sem, W, b, n, v, score)
            assert torch.equal(idx_v, idx) and torch.equal(sim_v.view(torch.int32), sim.view(torch.int32)) \
                and torch.equal(bg_v, bg), v


@pytest.mark.parametrize("S", [1, 8, 16])
def test_decode_split_lds_bound(S):
    """SPLIT_MAX codes on the split kernel, one more on the fp32 kernel: both decode correctly (one more used to be
    refused)."""
    dev = torch.device("cuda")
    for n, want in ((SPLIT_MAX, "split"), (SPLIT_MAX + 1, "fp32")):
        assert R.decode_path(S, n, 1, K)[0] == want
        for HW in (65, 4099):
            sem, W, b = random_problem(S, HW, n, _seed((S, n, HW, "lds")), dev)
            check_decode(sem, W, b, n, 1, scores(n, dev, 4))


@pytest.mark.parametrize("S,variant", [(32, 1), (16, 0), (16, 1), (4, 1)])
def test_decode_fp32_lds_bound(S, variant):
    """The largest code book at S decodes; one more code is refused with the message and nothing written."""
    dev = torch.device("cuda")
    n = R.max_codes(S, K)
    sem, W, b = random_problem(S, 333, n + 1, _seed((S, n, "max")), dev)
    check_decode(sem, W[:n].contiguous(), b[:n].contiguous(), n, variant, scores(n, dev, 5))
    score = scores(n + 1, dev, 6)
    rc, sim, idx, bg = decode(sem, W, b, n + 1, variant, score)
    assert rc < 0 and "too large for LDS" in _lib().last_error()
    assert torch.isnan(sim).all() and (idx == IDX_SENTINEL).all() and (bg == BG_SENTINEL).all()


LADDER_K = (3, 4, 8, 32, 256)


@pytest.mark.parametrize("variant,S", PATHS)
def test_decode_near_tie_ladder(variant, S):
    """Code 20 beats code 7 by exactly k e_p at every pixel: code 20 must win, for every rung k."""
    dev = torch.device("cuda")
    n = 37
    path = R.decode_path(S, n, variant, K)
    g = R.gamma(path, S)
    for k in LADDER_K:
        sem, W, b = R.ladder_problem(S, n, k, g, 777, _seed((S, k, "ladder")))
        ratio = R.ladder_ratio(sem, W, b, g)
        assert ratio.min() > 2.5, (k, ratio.min())
        t = [torch.from_numpy(x).to(dev) for x in (sem, W, b)]
        idx, _, _ = check_decode(*t, n, variant, scores(n, dev, 7))
        assert (idx == 20).all(), (k, int((idx != 20).sum()))


@pytest.mark.parametrize("variant,S", PATHS)
def test_decode_exact_ties_take_the_lowest_index(variant, S):
    """Duplicate (W row, bias) pairs: same lane of two 16-code blocks, two lanes of one block, first and last code."""
    dev = torch.device("cuda")
    for n, (i, j) in ((37, (3, 19)), (37, (3, 5)), (301, (1, 300)), (17, (1, 16)), (300, (13, 290))):
        sem, W, b = random_problem(S, 1000, n, _seed((S, n, i, j, "tie")), dev)
        W *= 0.01
        b *= 0.01
        W[j] = W[i]
        b[i] = b[j] = 10.0
        idx, _, _ = check_decode(sem, W, b, n, variant, scores(n, dev, 8))
        assert (idx == i).all(), (n, i, j, idx.unique().tolist())


@pytest.mark.parametrize("variant,S", PATHS)
def test_decode_zero_features(variant, S):
    """All features 0: with a zero bias every code ties (code 0 wins); with a bias its first maximum wins."""
    dev = torch.device("cuda")
    for n in (1, 17, 300):
        sem, W, b = random_problem(S, 130, n, _seed((S, n, "zero")), dev)
        sem.zero_()
        idx, _, _ = check_decode(sem, W, torch.zeros_like(b), n, variant, scores(n, dev, 9))
        assert (idx == 0).all()
        if n > 9:
            b[5] = b[9] = b.max() + 1
        idx, _, _ = check_decode(sem, W, b, n, variant, scores(n, dev, 9))
        assert (idx == int(b.argmax())).all()


@pytest.mark.parametrize("variant,S", PATHS)
def test_decode_all_negative_logits_never_pick_padding(variant, S):
    """Every real logit is negative and n_codes % 16 != 0: a padding code must never win."""
    dev = torch.device("cuda")
    for n in (1, 15, 17, 37, 301):
        sem, W, b = random_problem(S, 1000, n, _seed((S, n, "neg")), dev)
        W *= 0.01
        b = -100 - b.abs()
        idx, _, _ = check_decode(sem, W, b, n, variant, scores(n, dev, 10))
        assert (idx < n).all()


@pytest.mark.parametrize("variant,S", PATHS)
def test_decode_mixed_magnitudes(variant, S):
    """Features, weights and biases scaled by 2^k, k in -20 .. 20 element by element: the split is exact in every
    exponent range."""
    dev = torch.device("cuda")
    n = 45
    sem, W, b = random_problem(S, 2000, n, _seed((S, "mixed")), dev)
    g = torch.Generator(device="cpu").manual_seed(_seed((S, "exp")))
    e = lambda *shape: torch.exp2(torch.randint(-20, 21, shape, generator=g).float()).to(dev)  # noqa: E731
    check_decode(sem * e(S, 2000), W * e(n, S), b * e(n), n, variant, scores(n, dev, 11))


@pytest.mark.parametrize("variant,S", [(1, 16), (2, 5), (3, 9), (0, 16), (1, 32)])
def test_decode_thresholds_and_optional_outputs(variant, S):
    """A score equal to thresh is not background, a NaN score is not background and stays NaN; every NULL / non-NULL
    combination of the three outputs and of code_score writes exactly what was asked."""
    dev = torch.device("cuda")
    n, HW = 40, 517
    sem, W, b = random_problem(S, HW, n, _seed((S, "thr")), dev)
    score = scores(n, dev, 12)
    thresh = float(score[3])
    score[7] = float("nan")
    rc, sim, idx, bg = decode(sem, W, b, n, variant, score, thresh)
    assert rc == 0
    R.decode_check(sem, W, b, idx, R.gamma(R.decode_path(S, n, variant, K), S))
    R.decode_outputs_check(idx, score, thresh, sim, bg)
    # the fixture reaches the cases it is about
    picked = set(idx.unique().tolist())
    assert len(picked) > 10
    # codes 3 and 7 each take over the winner of a pixel, one better (two distinct winners other than 3 and 7)
    w3 = int(idx[(idx != 3) & (idx != 7)][0])
    w7 = int(idx[(idx != 3) & (idx != 7) & (idx != w3)][0])
    W[3], b[3], W[7], b[7] = W[w3].clone(), b[w3] + 1, W[w7].clone(), b[w7] + 1
    rc, sim, idx, bg = decode(sem, W, b, n, variant, score, thresh)
    assert rc == 0 and {3, 7} <= set(idx.unique().tolist())
    R.decode_outputs_check(idx, score, thresh, sim, bg)
    assert not bg[idx == 3].any() and (sim[idx == 3] == thresh).all()
    assert not bg[idx == 7].any() and torch.isnan(sim[idx == 7]).all()
    for table in (score, None):
        for mask in range(8):
            outs = tuple(o for o, bit in (("sim", 1), ("idx", 2), ("bg", 4)) if mask & bit)
            rc, s2, i2, b2 = decode(sem, W, b, n, variant, table, thresh, outputs=outs)
            assert rc == 0, _lib().last_error()
            R.decode_outputs_check(idx, table, thresh, s2, b2)
            if i2 is not None:
                assert torch.equal(i2, idx)


# ---- row pass -------------------------------------------------------------------------------------------------------
ROW_C = (1, 63, 64, 65, 128, 129, 191, 192, 193, 256, 257, 320, 321, 383, 384, 385, 448, 449, 511, 512)
ROW_S = (1, 3, 8, 15, 16)
ROW_HW = (1, 63, 64, 65)
N_WAVES = K["ROW_WAVES"]


def rows(inp, C, S, t, HW):
    """One goi_codebook_loss_rows call on NaN-filled outputs with a tail element; returns (rc, dsim, dsem, partials)."""
    L = _lib()
    dev = inp["sim_raw"].device
    width = R.row_width(C, S)
    dsim = torch.full((HW * C + 1,), float("nan"), device=dev)
    dsem = torch.full((S * HW + 1,), float("nan"), device=dev)
    part = torch.full((N_WAVES * width + 1,), float("nan"), device=dev)
    assert L.load().goi_codebook_loss_partial_rows() == N_WAVES
    rc = L.load().goi_codebook_loss_rows(_ptr(inp["sim_raw"]), _ptr(inp["inv_gnorm"]), _ptr(inp["sem"]), _ptr(inp["W"]),
                                         _ptr(inp["b"]), HW, C, S, float(t), _ptr(dsim), _ptr(dsem), _ptr(part), None)
    torch.cuda.synchronize()
    for tname, tt in (("dsim", dsim), ("dsem", dsem), ("partials", part)):
        assert torch.isnan(tt[-1]), f"{tname}: write past the end"
    return rc, dsim[:-1].view(HW, C), dsem[:-1].view(S, HW), part[:-1].view(N_WAVES, width)


def check_rows(HW, C, S, bias, t, seed):
    inp = R.make_rows_inputs(HW, C, S, bias, seed, device="cuda")
    rc, dsim, dsem, part = rows(inp, C, S, t, HW)
    assert rc == 0, _lib().last_error()
    worst = R.rows_check(inp["sim_raw"], inp["inv_gnorm"], inp["sem"], inp["W"], inp["b"], t, N_WAVES, dsim, dsem, part)
    for k, v in worst.items():
        _note(f"rows {k}", v)


@pytest.mark.parametrize("C", ROW_C)
def test_rows_every_codes_per_lane(C):
    """Each C at a CPL edge, ragged 64-pixel chunks; S, bias and t rotate with C."""
    i = ROW_C.index(C)
    for j, HW in enumerate(ROW_HW):
        S = ROW_S[(i + j) % len(ROW_S)]
        check_rows(HW, C, S, bias=(i + j) % 2 == 0, t=1.0 + (i + j // 2) % 2, seed=_seed((C, HW, S)))


@pytest.mark.parametrize("S", ROW_S)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("t", [1.0, 2.0])
def test_rows_channels_bias_anneal(S, bias, t):
    for C in (65, 449):
        check_rows(130, C, S, bias, t, _seed((S, bias, t, C)))


@pytest.mark.parametrize("C,S", [(64, 16), (193, 3), (320, 8), (385, 16), (512, 15)])
def test_rows_one_chunk_past_every_wave(C, S):
    """64 x waves + 1 pixels: wave 0 takes a second chunk of one pixel."""
    check_rows(64 * N_WAVES + 1, C, S, True, 2.0, _seed((C, S, "waves")))


def test_rows_large():
    check_rows(4 * 64 * N_WAVES + 333, 193, 16, True, 1.0, _seed("large"))


@pytest.mark.parametrize("S,C", [(17, 64), (0, 64), (8, 513), (8, 0), (16, 1024)])
def test_rows_refuse_bad_sizes(S, C):
    dev = torch.device("cuda")
    inp = R.make_rows_inputs(65, 64, 16, True, 1, device=dev)
    out = torch.full((1 << 20,), float("nan"), device=dev)
    rc = _lib().load().goi_codebook_loss_rows(_ptr(inp["sim_raw"]), _ptr(inp["inv_gnorm"]), _ptr(inp["sem"]),
                                              _ptr(inp["W"]), _ptr(inp["b"]), 65, C, S, 1.0, _ptr(out), _ptr(out),
                                              _ptr(out), None)
    torch.cuda.synchronize()
    assert rc < 0 and "1 <= S <= 16, 1 <= C <= 512" in _lib().last_error()
    assert torch.isnan(out).all()
