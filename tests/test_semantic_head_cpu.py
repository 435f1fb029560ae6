"""CPU checks that keep tests/test_gpu_semantic_head.py honest (no GPU needed):
  * the bounds it straddles parse out of the kernel sources, and its case tables straddle every one of them --
    retuning a bound fails here instead of silently losing coverage;
  * its checkers fail on each kind of wrong answer a broken kernel would give, and the row-pass reference agrees
    with autograd on the loss it differentiates;
  * the entry points refuse bad arguments before any HIP call.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import semantic_head_reference as R
from tests import test_gpu_semantic_head as G

K = R.kernel_constants()


# ---- constants and tables -------------------------------------------------------------------------------------------
def test_kernel_constants_parse():
    assert K["SPLIT_LDS"] == 64 * 1024 and K["FP32_LDS"] == 160 * 1024 and K["SPLIT_S_MAX"] == 16
    assert R.split_max_codes(K) == 576 and R.split_lds(577) > K["SPLIT_LDS"] >= R.split_lds(576)
    assert R.max_codes(16, K) == 2400 and R.max_codes(32, K) == 1232 and R.max_codes(1, K) == 8192
    for S in range(1, 33):
        n = R.max_codes(S, K)
        assert R.fp32_lds(S, n) <= K["FP32_LDS"] < R.fp32_lds(S, n + 1)
    assert K["GRID_CAP"] == 2048 and (K["FIXED_K4"], K["FIXED_NBLK"]) == (4, 19)
    assert K["ROW_S_MAX"] == 16 and K["ROW_C_MAX"] == 512 and K["ROW_WAVES"] == 2048
    assert K["ROW_CPL"] == list(range(1, K["ROW_C_MAX"] // 64 + 1)) and 1 <= K["ROW_CPL_2WG"] < max(K["ROW_CPL"])


def test_decode_tables_reach_every_instantiation():
    paths = {R.decode_path(S, 37, v, K) for v, S in G.PATHS}
    assert {("split", npb) for npb in (1, 2, 4)} <= paths
    assert {("fp32", k4, 0) for k4 in range(1, 9)} <= paths
    assert R.decode_path(16, 300, 0, K) == ("fp32", 4, 19)
    # S around the split kernel's 8-channel halves and its bound, in every variant
    assert {(1, 7), (1, 8), (1, 9), (1, 16), (1, 17)} <= set(G.PATHS)


def test_decode_tables_straddle_every_threshold():
    hw = set(G.HW_EDGES)
    for unit in (16, 32, 64):  # 16-pixel block, 16 NPB-pixel units, 64-pixel group
        assert {unit - 1, unit, unit + 1} <= hw
    assert 1 in hw
    assert G.TRIP == K["GRID_CAP"] * 256
    codes = set(G.CODE_EDGES)
    assert {1, 15, 16, 17} <= codes
    nblk = {(n + 15) // 16 for n in codes | {288}}
    assert any(x % 2 for x in nblk) and any(x % 2 == 0 for x in nblk)  # the split kernel's unroll by two
    assert G.SPLIT_MAX == R.split_max_codes(K)
    assert R.decode_path(16, G.SPLIT_MAX, 1, K)[0] == "split" and R.decode_path(16, G.SPLIT_MAX + 1, 1, K)[0] == "fp32"
    assert R.decode_path(32, R.max_codes(32, K) + 1, 1, K) is None


def test_row_tables_straddle_every_threshold():
    cs = set(G.ROW_C)
    for cpl in K["ROW_CPL"]:
        assert {64 * (cpl - 1) + 1, 64 * cpl} <= cs, cpl
    assert K["ROW_C_MAX"] in cs and 64 * K["ROW_CPL_2WG"] + 1 in cs
    assert {1, 63, 64, 65} <= set(G.ROW_HW)
    assert set(G.ROW_S) >= {1, K["ROW_S_MAX"] - 1, K["ROW_S_MAX"]}
    assert G.N_WAVES == K["ROW_WAVES"]


# ---- the decode checkers fail on wrong answers ----------------------------------------------------------------------
def _t(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)) for x in xs]


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("k", [3, 4])
def test_ladder_catches_a_two_term_split(S, k):
    """At the low rungs the gap sits in the l part of the weight: a two-term split ties the two codes (and would keep
    the lower, worse one); the kernel's three-term split keeps the better one ahead; the checker refuses the worse."""
    path = ("split", 2)
    g = R.gamma(path, S)
    sem, W, b = R.ladder_problem(S, 37, k, g, 200, seed=S * 10 + k)
    ratio = R.ladder_ratio(sem, W, b, g)
    assert (abs(ratio - k) < 0.05 * k).all()
    l3 = R.split_logits(sem, W, b, terms=3)
    l2 = R.split_logits(sem, W, b, terms=2)
    assert (l3[:, 20] > l3[:, 7]).all()
    assert (l2[:, 20] <= l2[:, 7]).all()
    sem_t, W_t, b_t = _t(sem, W, b)
    R.decode_check(sem_t, W_t, b_t, torch.full((200,), 20), g)
    with pytest.raises(AssertionError, match="below the best logit"):
        R.decode_check(sem_t, W_t, b_t, torch.full((200,), 7), g)


def test_ladder_rungs_hit_their_ratio_on_every_path():
    for v, S in G.PATHS:
        g = R.gamma(R.decode_path(S, 37, v, K), S)
        for k in G.LADDER_K:
            sem, W, b = R.ladder_problem(S, 37, k, g, 100, seed=k)
            ratio = R.ladder_ratio(sem, W, b, g)
            assert (abs(ratio - k) < 0.05 * k).all(), (v, S, k)


def test_decode_checker_refuses_highest_index_on_a_tie_and_padding():
    torch.manual_seed(0)
    sem, W, b = torch.randn(8, 50), torch.randn(37, 8) * 0.01, torch.zeros(37)
    W[19], b[3], b[19] = W[3], 10.0, 10.0
    R.decode_check(sem, W, b, torch.full((50,), 3), R.gamma(("split", 2), 8))
    with pytest.raises(AssertionError, match="identical lower twin"):
        R.decode_check(sem, W, b, torch.full((50,), 19), R.gamma(("split", 2), 8))
    with pytest.raises(AssertionError, match="out of"):
        R.decode_check(sem, W, b, torch.full((50,), 37), R.gamma(("split", 2), 8))


def test_decode_output_checker_refuses_wrong_scores():
    idx = torch.tensor([0, 1, 2, 3])
    score = torch.tensor([0.2, 0.5, 0.9, float("nan")])
    sim = torch.tensor([0.0, 0.5, 0.9, float("nan")])
    bg = torch.tensor([1, 0, 0, 0], dtype=torch.uint8)
    R.decode_outputs_check(idx, score, 0.5, sim, bg)
    with pytest.raises(AssertionError, match="sim differs"):
        R.decode_outputs_check(idx, score, 0.5, torch.tensor([0.2, 0.5, 0.9, float("nan")]), bg)  # not zeroed
    with pytest.raises(AssertionError, match="bg differs"):
        R.decode_outputs_check(idx, score, 0.5, sim, torch.tensor([1, 1, 0, 0], dtype=torch.uint8))  # == thresh is fg
    with pytest.raises(AssertionError, match="bg differs"):
        R.decode_outputs_check(idx, score, 0.5, sim, torch.tensor([1, 0, 0, 1], dtype=torch.uint8))  # NaN is fg
    R.decode_outputs_check(idx, None, 0.5, torch.zeros(4), torch.ones(4, dtype=torch.uint8))  # no table: score 0
    R.decode_outputs_check(idx, None, -0.5, torch.zeros(4), torch.zeros(4, dtype=torch.uint8))


# ---- the row-pass reference and its checker -------------------------------------------------------------------------
def _autograd_rows(inp, t):
    """The loss of the codebook_loss.hip header, differentiated by autograd in float64 (label and arg-maxima fixed)."""
    sim, inv, sem, W, b = inp["sim_raw"], inp["inv_gnorm"], inp["sem"], inp["W"], inp["b"]
    HW, C = sim.shape
    xs32 = sim * inv[:, None]
    xs = xs32.double().requires_grad_()
    f = sem.double().T.clone().requires_grad_()
    W64 = W.double().clone().requires_grad_()
    b64 = (b if b is not None else torch.zeros(C)).double().clone().requires_grad_()
    z = f @ W64.T + b64
    P = torch.softmax(z, 1)
    label = (xs32 == xs32.amax(1, keepdim=True)).double()
    lab = 50 * ((P - label) ** 2).mean()
    m = xs.gather(1, xs.detach().argmax(1, keepdim=True))[:, 0]
    sl = 1 - m.mean()
    recc = 1 - xs.gather(1, z.detach().argmax(1, keepdim=True))[:, 0].mean()
    q = torch.softmax(t * xs, 1)
    sl1 = (-(q * torch.log_softmax(t * xs, 1)).sum(1)).mean()
    (lab + sl + 0.3 * sl1 + recc).backward()
    return xs.grad * inv.double()[:, None], f.grad.T, W64.grad, b64.grad


@pytest.mark.parametrize("C,S,bias,t", [(1, 1, True, 1.0), (65, 3, True, 2.0), (130, 16, False, 1.0), (7, 8, True, 2.0)])
def test_row_reference_matches_autograd(C, S, bias, t):
    inp = R.make_rows_inputs(150, C, S, bias, seed=C + S)
    dsim, dsem, part = R.rows_expected(inp["sim_raw"], inp["inv_gnorm"], inp["sem"], inp["W"], inp["b"], t, 4)
    gs, gf, gW, gb = _autograd_rows(inp, t)
    assert torch.allclose(dsim, gs, rtol=1e-12, atol=1e-15)
    assert torch.allclose(dsem, gf, rtol=1e-12, atol=1e-15)
    tot = part.sum(0)[:C * (S + 1)].view(C, S + 1)
    assert torch.allclose(tot[:, :S], gW, rtol=1e-12, atol=1e-15)
    if bias:
        assert torch.allclose(tot[:, S], gb, rtol=1e-12, atol=1e-15)


def _rows_case(C=70, S=5, HW=150, seed=3, t=2.0):
    inp = R.make_rows_inputs(HW, C, S, True, seed)
    want = R.rows_expected(inp["sim_raw"], inp["inv_gnorm"], inp["sem"], inp["W"], inp["b"], t, 8)
    return inp, [w.float() for w in want], t


def _check(inp, t, dsim, dsem, part):
    return R.rows_check(inp["sim_raw"], inp["inv_gnorm"], inp["sem"], inp["W"], inp["b"], t, 8, dsim, dsem, part)


def test_row_checker_accepts_the_rounded_reference():
    inp, (dsim, dsem, part), t = _rows_case()
    worst = _check(inp, t, dsim, dsem, part)
    assert all(v < 0.5 for v in worst.values()), worst


def test_row_checker_refuses_a_label_set_missing_one_tie():
    inp, (dsim, dsem, part), t = _rows_case()
    xs = inp["sim_raw"] * inp["inv_gnorm"][:, None]
    p = int(((xs == xs.amax(1, keepdim=True)).sum(1) == 3).nonzero()[0])
    tied = (xs[p] == xs[p].max()).nonzero()[:, 0]
    bad = {k: (v.clone() if v is not None else None) for k, v in inp.items()}
    bad["sim_raw"][p, tied[-1]] = torch.nextafter(bad["sim_raw"][p, tied[-1]], torch.tensor(-1e30))
    wrong = [w.float() for w in R.rows_expected(bad["sim_raw"], bad["inv_gnorm"], bad["sem"], bad["W"], bad["b"], t, 8)]
    with pytest.raises(AssertionError):
        _check(inp, t, *wrong)


def test_row_checker_refuses_a_nan_partial_row_and_stray_values():
    inp, (dsim, dsem, part), t = _rows_case()
    for mutate in (lambda d, e, q: q[5].fill_(float("nan")),            # a wave without pixels left unwritten
                   lambda d, e, q: q[1, 3].fill_(float("nan")),          # one dW element
                   lambda d, e, q: q[0, -1].mul_(1 + 1e-3),              # sim-at-arg_a sum
                   lambda d, e, q: d[7, 69].fill_(float("nan")),         # a dsim element
                   lambda d, e, q: e[4, 100].mul_(1 + 1e-3),             # a dsem element
                   lambda d, e, q: d[3].copy_(d[3].flip(0))):            # arg_a / arg_s taken elsewhere
        d, e, q = dsim.clone(), dsem.clone(), part.clone()
        mutate(d, e, q)
        with pytest.raises(AssertionError):
            _check(inp, t, d, e, q)


def test_row_checker_refuses_last_maximum_for_arg_a():
    """Decoder ties are exact on the dyadic grid: taking the last maximum moves dsim and the sim-at-arg_a sum."""
    inp, (dsim, dsem, part), t = _rows_case()
    z = inp["sem"].double().T @ inp["W"].double().T + inp["b"].double()
    last = z.shape[1] - 1 - z.flip(1).argmax(1)
    assert (last != z.argmax(1)).any()
    xs = (inp["sim_raw"] * inp["inv_gnorm"][:, None]).double()
    d = dsim.clone().double()
    HW = xs.shape[0]
    rows = torch.arange(HW)
    d[rows, z.argmax(1)] += inp["inv_gnorm"].double() / HW
    d[rows, last] -= inp["inv_gnorm"].double() / HW
    q = part.clone().double()
    q[:, -1] = 0
    q[:, -1].index_add_(0, (rows // 64) % 8, xs[rows, last])
    with pytest.raises(AssertionError):
        _check(inp, t, d.float(), dsem, q.float())


# ---- host refusals (they return before any HIP call) -----------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


FAKE = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first


def _err(lib):
    return lib.goi_raster_last_error().decode()


def _decode(lib, S=16, HW=1, n=37, null=()):
    p = {k: (None if k in null else FAKE) for k in ("sem", "W", "b", "score", "sim", "idx", "bg")}
    return lib.goi_semantic_decode(p["sem"], S, HW, p["W"], p["b"], n, p["score"], 0.5, p["sim"], p["idx"], p["bg"], None)


def test_decode_refuses_bad_arguments(lib):
    for S, n, HW in ((0, 37, 1), (33, 37, 1), (16, 0, 1), (16, 37, -1)):
        assert _decode(lib, S=S, n=n, HW=HW) < 0 and "1 <= S <= 32" in _err(lib)
    for name in ("sem", "W", "b"):
        assert _decode(lib, null=(name,)) < 0 and "NULL" in _err(lib)
    for S in (1, 4, 5, 16, 17, 32):
        for v in (0, 1):
            from goi_hyperplane_amd import _lib as L
            L.set_option("decode_variant", v)
            try:
                assert _decode(lib, S=S, n=R.max_codes(S, K) + 1) < 0 and "too large for LDS" in _err(lib)
            finally:
                L.set_option("decode_variant", 1)
    assert _decode(lib, HW=0, n=100000) == 0  # nothing to do


def _rows(lib, S=8, C=64, HW=65, null=()):
    p = {k: (None if k in null else FAKE) for k in ("sim", "inv", "sem", "W", "b", "dsim", "dsem", "part")}
    return lib.goi_codebook_loss_rows(p["sim"], p["inv"], p["sem"], p["W"], p["b"], HW, C, S, 1.0, p["dsim"], p["dsem"],
                                      p["part"], None)


def test_rows_refuse_bad_arguments(lib):
    for S, C in ((0, 64), (17, 64), (8, 0), (8, 513), (-1, 1)):
        assert _rows(lib, S=S, C=C) < 0 and "1 <= S <= 16, 1 <= C <= 512" in _err(lib)
    assert _rows(lib, HW=-1) < 0 and "bad HW" in _err(lib)
    for name in ("sim", "inv", "sem", "W", "dsim", "dsem", "part"):
        assert _rows(lib, null=(name,)) < 0 and "NULL" in _err(lib), name
    assert lib.goi_codebook_loss_partial_rows() == K["ROW_WAVES"]
