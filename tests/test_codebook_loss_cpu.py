"""CPU checks that keep tests/test_gpu_codebook_loss.py honest (no GPU needed):
  * the fused path's bounds parse out of csrc/codebook_loss.hip and the GPU tables straddle every one of them;
  * the split-product term of the error model bounds what three bf16 partial products drop;
  * the fused reference agrees with autograd of semantic.codebook_losses run in float64;
  * every checker refuses each kind of wrong result a broken kernel would give;
  * the entry points refuse bad shapes before any HIP call.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from tests import codebook_loss_reference as CR
from tests import test_gpu_codebook_loss as G
from tests.semantic_head_reference import bf16_rne

K = CR.fused_constants()


# ---- constants and tables ---------------------------------------------------------------------------------------------
def test_fused_constants_parse():
    assert (K["NCB"], K["NC"], K["D"], K["SIM_KC"]) == (19, 304, 256, 32)
    assert (K["FU_WG_PIX"], K["BLOCK"], K["FU_TIE_WORDS"], K["FU_NJ"]) == (128, 16, 10, 10)
    assert (K["GD_WAVES"], K["DS_WAVES"], K["DLUT_BLOCKS"], K["DL2_PIX"], K["DL_KP"]) == (2048, 8192, 256, 32, 32)
    assert (K["C_MIN"], K["S_MAX"], K["HW_MIN"], K["HW_LIMIT"], K["SIM_WG_PIX"]) == (289, 16, 4, 1 << 25, 128)
    assert 32 * K["FU_TIE_WORDS"] >= K["NC"] > 32 * (K["FU_TIE_WORDS"] - 1)


def _straddles(values, edge, step=4):
    return {edge, edge + step} <= set(values)


def test_fused_tables_straddle_every_threshold():
    hw = G.FUSED_HW
    assert min(hw) == K["HW_MIN"] and all(x % 4 == 0 and x < K["HW_LIMIT"] for x in hw)
    for edge in (K["BLOCK"], K["FU_WG_PIX"],                  # one 16-pixel block, one codebook_simgrad_k workgroup
                 K["DLUT_BLOCKS"] * K["DL2_PIX"],              # one trip of codebook_dlut2_k
                 K["GD_WAVES"] * K["BLOCK"],                   # one trip of decoder_gd_k
                 K["DS_WAVES"] * K["BLOCK"]):                  # one trip of decoder_stats_k
        assert _straddles(hw, edge), edge
    assert {K["BLOCK"] - 4, K["FU_WG_PIX"] - 4} <= set(hw)
    # several trips of every persistent kernel, and the headline frame
    assert any(x > 2 * K["DS_WAVES"] * K["BLOCK"] and x != G.HEADLINE for x in hw) and G.HEADLINE in hw
    assert G.TIES_HW > K["GD_WAVES"] * K["BLOCK"] and G.TIES_HW > K["DLUT_BLOCKS"] * K["DL2_PIX"]
    assert set(G.FUSED_C) == set(range(K["NC"] - 15, K["NC"] + 1)) and K["C_MIN"] == K["NC"] - 15
    S = {i % 16 + 1 for i in range(len(G.FUSED_C))} | {16 - i % 16 for i in range(len(G.FUSED_C))}
    assert S == set(range(1, K["S_MAX"] + 1))
    assert G.REFUSE_HW == K["HW_LIMIT"]


def test_tie_groups_reach_every_tie_mask_case():
    for Cn in G.FUSED_C:
        groups = CR.tie_groups(Cn)
        flat = [c for grp in groups for c in grp]
        assert len(flat) == len(set(flat)) and max(flat) < Cn
        assert any(len({c // 16 for c in grp}) == 1 for grp in groups)                        # one 16-code block
        assert any(len({c % 16 for c in grp}) == 1 and len({c // 16 for c in grp}) > 1 for grp in groups)  # one lane
        assert any(len({c // 32 for c in grp}) > 1 and {31, 32} <= set(grp) for grp in groups)  # tie mask word edge
        assert any(c >= 16 * (K["NCB"] - 1) for c in flat)                                  # the padded last block
        assert any(c // 32 == K["FU_TIE_WORDS"] - 1 for c in flat)                            # the last mask word
        assert {len(grp) for grp in groups} == {2, 3}


def test_dlut_and_sim_tables_straddle_every_threshold():
    assert {K["C_MIN"], K["NC"]} <= set(G.DLUT_C) and all(K["C_MIN"] <= c <= K["NC"] for c in G.DLUT_C)
    hw = set(G.DLUT_HW)
    assert {K["DL_KP"] - 4, K["DL_KP"], K["DL_KP"] + 4} <= hw          # one stage, a ragged second range
    trip = K["DLUT_BLOCKS"] * K["DL_KP"]                               # beyond: every range has several stages
    assert {trip, trip + 4} <= hw and G.HEADLINE in hw and any(trip < x < G.HEADLINE for x in hw - {trip + 4})
    assert 4 in hw
    sw = K["SIM_WG_PIX"]
    assert {sw - 1, sw, sw + 1, 2 * sw - 1, 2 * sw + 1} <= set(G.SIM_HW) and 1 in G.SIM_HW
    assert {4, 16, 64, K["NC"] - 4, K["NC"]} <= set(G.SIM_C) and all(c % 4 == 0 for c in G.SIM_C)


def test_mappings():
    assert CR.fused_blocks(4, K) == 8 and CR.fused_blocks(132, K) == 16
    nb = CR.gd_blocks_per_wave(131076, K)
    assert int(nb.sum()) == CR.fused_blocks(131076, K) and int(nb.max()) == 5 and int(nb.min()) == 4
    blen, ranges = CR.dlut2_ranges(8196, K)
    assert blen == 64 and ranges[0] == (0, 64) and ranges[128] == (8192, 8196) and ranges[129] == (8196, 8196)
    per, ranges = CR.dlut_ranges(36, K)
    assert per == 32 and ranges[:3] == [(0, 32), (32, 36), (36, 36)]
    per, ranges = CR.dlut_ranges(8196, K)
    assert per == 64 and ranges[-1] == (8196, 8196)


# ---- the split-product term of the error model --------------------------------------------------------------------------
def test_split_product_bound():
    """hi*hi + lo*hi + hi*lo of the two-plane bf16 split is within SP |a||b| of a*b, and the bound is nearly reached."""
    rng = np.random.default_rng(7)
    n = 1 << 20
    a = (rng.uniform(1, 2, n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32) * rng.choice([-1, 1], n)
    b = (rng.uniform(1, 2, n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
    # worst cases: residuals of half a bf16 ulp in both planes
    a[:16] = np.float32(1 + 2 ** -8 + 2 ** -9 + 2 ** -17)
    b[:16] = np.float32(1 + 2 ** -8 + 2 ** -9 + 2 ** -17)

    def split(x):
        h = bf16_rne(x)
        return h.astype(np.float64), bf16_rne((x - h).astype(np.float32)).astype(np.float64)

    (ah, al), (bh, bl) = split(a), split(b)
    got = ah * bh + al * bh + ah * bl          # exact in float64 (8 x 8 significant bits each)
    err = np.abs(got - a.astype(np.float64) * b.astype(np.float64)) / np.abs(a.astype(np.float64) * b)
    assert err.max() <= CR.SP
    assert err.max() > 0.3 * CR.SP


# ---- the fused reference against autograd ------------------------------------------------------------------------------
@contextlib.contextmanager
def _float64_restatement():
    """semantic.codebook_losses casts the ground truth and the label with .float(); run in float64, those casts give
    float64."""
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double(*a, **k)
    try:
        yield
    finally:
        torch.Tensor.float = orig


def _autograd_fused(inp, t, H, W_):
    from goi_hyperplane_amd.semantic import SemanticModel, codebook_losses
    g, l1, sem, W, b = (inp[k] for k in ("g", "l1", "sem", "W", "b"))
    S, HW = sem.shape
    Cn, D = l1.shape
    mlp = SemanticModel(dim_in=S, dim_out=Cn, num_layer=1, use_bias=b is not None, device="cpu").double()
    with torch.no_grad():
        mlp.layers[0].weight.copy_(W.double())
        if b is not None:
            mlp.layers[0].bias.copy_(b.double())
    scale = torch.linspace(0.5, 2.0, Cn, dtype=torch.float64)[CR.first_duplicate_rows(l1)]  # duplicates stay duplicates
    lut = (l1.double() * scale[:, None]).requires_grad_()
    f = sem.double().reshape(S, H, W_).clone().requires_grad_()
    with _float64_restatement():
        loss, terms = codebook_losses(f, mlp, lut, g.double().reshape(D, H, W_), 10 if t == 1.0 else 2000)
    loss.backward()
    lin = mlp.layers[0]
    return terms, f.grad.reshape(S, HW), lin.weight.grad, (lin.bias.grad if b is not None else None), lut


@pytest.mark.parametrize("Cn,S,bias,t,decoder,ties", [(300, 16, True, 1.0, "dyadic", True), (289, 1, True, 2.0, "general", False),
                                                      (304, 5, False, 2.0, "general", True), (296, 9, False, 1.0, "dyadic", False)])
def test_fused_reference_matches_autograd(Cn, S, bias, t, decoder, ties):
    H, W_ = 8, 12
    HW = H * W_
    inp = CR.make_fused_inputs(HW, Cn, S, bias, Cn + S, decoder=decoder, ties=ties, K=K)
    terms, gsem, gW, gb, lut = _autograd_fused(inp, t, H, W_)
    lut1 = (lut / lut.norm(dim=1, keepdim=True)).detach()
    ref = CR.fused_reference(inp["g"], lut1, inp["sem"], inp["W"], inp["b"], t, K)
    if ties:
        raw = inp["g"].double().T @ lut1.T
        assert ((raw == raw.amax(1, keepdim=True)).sum(1) > 1).sum() > HW // 4  # the restatement sees the ties too

    def close(a, b):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-13 * float(b.abs().max())), float((a - b).abs().max())

    close(ref["dsem"], gsem)
    tot = ref["partials"].sum(0)
    nd = Cn * (S + 1)
    dWb = tot[:nd].view(Cn, S + 1)
    close(dWb[:, :S], gW)
    if bias:
        close(dWb[:, S], gb)
    sums = tot[nd:]
    close(torch.stack([sums[0] * 50 / (HW * Cn), 1 - sums[1] / HW, sums[2] / HW, 1 - sums[3] / HW]),
          torch.stack([terms[k].detach() for k in ("lab", "sl", "sl1", "recc")]))
    dl1 = ref["dlut"].sum(0)
    dlut = (dl1 - lut1 * (lut1 * dl1).sum(1, keepdim=True)) / lut.detach().norm(dim=1, keepdim=True)
    close(dlut, lut.grad)


# ---- the checkers fail on wrong results -----------------------------------------------------------------------------------
HW_CASE, C_CASE, S_CASE, T_CASE = 8196, 300, 5, 2.0  # two 32-pixel chunks per codebook_dlut2_k workgroup


@pytest.fixture(scope="module")
def case():
    inp = CR.make_fused_inputs(HW_CASE, C_CASE, S_CASE, True, 11, decoder="dyadic", ties=True, K=K)
    ref = CR.fused_reference(inp["g"], inp["l1"], inp["sem"], inp["W"], inp["b"], T_CASE, K)
    dl = torch.zeros(K["DLUT_BLOCKS"], K["NC"], K["D"])
    dl[:ref["dlut"].shape[0], :C_CASE] = ref["dlut"].float()
    got = dict(dsem=ref["dsem"].float(), partials=ref["partials"].float(), dlut=dl)
    return inp, ref, got


def _check(inp, got, **kw):
    return CR.fused_check(inp["g"], inp["l1"], inp["sem"], inp["W"], inp["b"], T_CASE, got["dsem"], got["partials"],
                          got["dlut"], K, **kw)


def _copy(got):
    return {k: v.clone() for k, v in got.items()}


def test_fused_checker_accepts_the_rounded_reference(case):
    inp, ref, got = case
    worst = _check(inp, got)
    assert all(v < 0.5 for v in worst.values()), worst
    assert _check(inp, got, chunk_px=64) == worst  # the chunking does not change what is checked


def test_fused_checker_refuses_a_dlut_row_off_by_three_tolerances(case):
    inp, ref, got = case
    bad = _copy(got)
    bad["dlut"][17, 201] += 3 * ref["t_dlut"][17, 201].float()
    with pytest.raises(AssertionError, match="dlut partials"):
        _check(inp, bad)


def _pixels(inp, p0, p1):
    first = CR.first_duplicate_rows(inp["l1"])
    return CR.fused_pixels(inp["g"][:, p0:p1], inp["l1"], first, inp["sem"][:, p0:p1], inp["W"], inp["b"], T_CASE,
                           HW_CASE, K)


def test_fused_checker_refuses_a_missing_dlut_chunk(case):
    """Workgroup 5 owns pixels 320 .. 383: its second 32-pixel chunk left out."""
    inp, ref, got = case
    blen, ranges = CR.dlut2_ranges(HW_CASE, K)
    assert ranges[5] == (320, 384) and blen == 2 * K["DL2_PIX"]
    r = _pixels(inp, 352, 384)
    bad = _copy(got)
    bad["dlut"][5, :C_CASE] -= (r["dsim"].T @ inp["g"][:, 352:384].double().T).float()
    with pytest.raises(AssertionError, match="dlut partials"):
        _check(inp, bad)


def test_fused_checker_refuses_a_pixel_missing_from_a_dw_row(case):
    inp, ref, got = case
    p = 1000
    r = _pixels(inp, p, p + 1)
    wave = (p // K["BLOCK"]) % K["GD_WAVES"]
    f1 = torch.cat([r["f"][0], torch.ones(1, dtype=torch.float64)])
    bad = _copy(got)
    bad["partials"][wave, :C_CASE * (S_CASE + 1)] -= (r["dz"][0][:, None] * f1[None, :]).flatten().float()
    with pytest.raises(AssertionError, match="partials \\(d"):
        _check(inp, bad)


def test_fused_checker_refuses_a_label_set_missing_one_tie(case):
    """Code 9 (tied with code 3) nudged below: the wrong results label 3 alone where that pair wins."""
    inp, ref, got = case
    l1 = inp["l1"].clone()
    l1[9, torch.argmax(l1[9].abs())] *= 1 - 2 ** -20
    wrong = CR.fused_reference(inp["g"], l1, inp["sem"], inp["W"], inp["b"], T_CASE, K)
    raw = inp["g"].double().T @ inp["l1"].double().T
    assert (raw.argmax(1) == 3).sum() > 10
    bad = _copy(got)
    bad["dsem"], bad["partials"] = wrong["dsem"].float(), wrong["partials"].float()
    with pytest.raises(AssertionError, match="dsem|partials"):
        _check(inp, bad)


def test_fused_checker_refuses_last_maximum_for_arg_a(case):
    """Decoder ties are exact on the dyadic grid: arg_a at the last maximum moves dsim (hence dLUT) and the sim-at-arg_a
    sum."""
    inp, ref, got = case
    z = inp["sem"].double().T @ inp["W"].double().T + inp["b"].double()
    first, last = z.argmax(1), z.shape[1] - 1 - z.flip(1).argmax(1)
    moved = (first != last).nonzero()[:, 0]
    assert moved.numel() > 10
    g64 = inp["g"].double()
    inv = g64.pow(2).sum(0).rsqrt()
    xs = (g64.T @ inp["l1"].double().T) * inv[:, None]
    blen, _ = CR.dlut2_ranges(HW_CASE, K)
    dl = got["dlut"].double()
    part = got["partials"].double()
    nd = C_CASE * (S_CASE + 1)
    for p in moved.tolist():
        w = inv[p] / HW_CASE * g64[:, p]
        dl[p // blen, first[p]] += w
        dl[p // blen, last[p]] -= w
        part[(p // K["BLOCK"]) % K["GD_WAVES"], nd + 3] += xs[p, last[p]] - xs[p, first[p]]
    for name, bad in (("dlut partials", dict(got, dlut=dl.float())),
                      ("loss sum sim_a", dict(got, partials=part.float()))):
        with pytest.raises(AssertionError, match=name):
            _check(inp, bad)


def test_fused_checker_refuses_a_nonzero_padded_code_row_and_nans(case):
    inp, ref, got = case
    n_dl = ref["dlut"].shape[0]
    nW_used = CR.fused_blocks(HW_CASE, K)
    for name, mutate in (("padded code rows", lambda d: d["dlut"][0, C_CASE, 7].fill_(1e-30)),
                         ("padded code rows", lambda d: d["dlut"][n_dl + 3, K["NC"] - 1, 0].fill_(-1e-30)),
                         ("without pixels", lambda d: d["dlut"][n_dl + 3, 0, 0].fill_(float("nan"))),
                         ("dlut partials", lambda d: d["dlut"][3, 5, 5].fill_(float("nan"))),
                         ("partials \\(dW\\)", lambda d: d["partials"][nW_used + 7, 0].fill_(float("nan"))),
                         ("partials \\(db\\)", lambda d: d["partials"][2, S_CASE].fill_(float("nan"))),
                         ("loss sum H", lambda d: d["partials"][7, -2].fill_(float("nan"))),
                         ("dsem", lambda d: d["dsem"][4, 8000].fill_(float("nan")))):
        bad = _copy(got)
        mutate(bad)
        with pytest.raises(AssertionError, match=name):
            _check(inp, bad)


def test_dlut_checker_refuses_a_missing_last_stage():
    """codebook_dlut_k at 8196 pixels: ranges of 64 pixels (two stages); each range without its last stage fails, the
    exact sums pass, as do the sums rounded to fp32."""
    HW, Cn = 8196, 301
    gen = torch.Generator().manual_seed(3)
    dsim = torch.randn(HW, Cn, generator=gen) / HW
    g = torch.randn(256, HW, generator=gen)
    val, tol = CR.dlut_reference(dsim, g, K)
    out = torch.zeros(K["DLUT_BLOCKS"], K["NC"], 256)
    out[:val.shape[0], :Cn] = val.float()
    assert CR.dlut_check(dsim, g, out, K) < 0.5
    per, ranges = CR.dlut_ranges(HW, K)
    assert per == 2 * K["DL_KP"]
    short = dsim.clone()
    for q0, q1 in ranges:
        if q1 - q0 > K["DL_KP"]:
            short[q0 + (q1 - q0 - 1) // K["DL_KP"] * K["DL_KP"]:q1] = 0
    v2, _ = CR.dlut_reference(short, g, K)
    bad = out.clone()
    bad[:v2.shape[0], :Cn] = v2.float()
    with pytest.raises(AssertionError, match="dlut ranges"):
        CR.dlut_check(dsim, g, bad, K)
    for mutate in (lambda o: o[0, Cn, 0].fill_(1e-30), lambda o: o[200, 0, 0].fill_(float("nan")),
                   lambda o: o[1, 7, 9].mul_(1 + 1e-4)):
        bad = out.clone()
        mutate(bad)
        with pytest.raises(AssertionError, match="dlut ranges"):
            CR.dlut_check(dsim, g, bad, K)


def test_sim_checker_refuses_wrong_elements():
    gen = torch.Generator().manual_seed(4)
    l1 = torch.randn(300, 256, generator=gen)
    l1 = l1 / l1.norm(dim=1, keepdim=True)
    g = torch.randn(256, 130, generator=gen)
    sim = (g.double().T @ l1.double().T).float()
    inv = g.double().pow(2).sum(0).rsqrt().float()
    ws, wi = CR.sim_check(g, l1, sim, inv, K)
    assert ws < 0.5 and wi < 0.5
    tol = CR.sim_tolerance_factor(K) * (g.double().abs().T @ l1.double().abs().T)
    for name, s2, i2 in (("sim_raw", sim.index_put((torch.tensor([5]), torch.tensor([299])),
                                                    (sim[5, 299] + 3 * tol[5, 299]).float()), inv),
                         ("sim_raw", sim.index_fill(0, torch.tensor([129]), float("nan")), inv),
                         ("inv_gnorm", sim, inv * (1 + 1e-5))):
        with pytest.raises(AssertionError, match=name):
            CR.sim_check(g, l1, s2, i2, K)


# ---- host refusals (they return before any HIP call) ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


FAKE = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first


def _err(lib):
    return lib.goi_raster_last_error().decode()


def test_fused_refuses_bad_shapes(lib):
    for HW, Cn, D, S in ((1 << 25, 300, 256, 16), (0, 300, 256, 16), (6, 300, 256, 16), (64, 288, 256, 16),
                         (64, 305, 256, 16), (64, 300, 128, 16), (64, 300, 256, 0), (64, 300, 256, 17)):
        rc = lib.goi_codebook_fused(FAKE, FAKE, FAKE, FAKE, None, HW, Cn, D, S, 1.0, FAKE, FAKE, FAKE, FAKE, None)
        assert rc < 0 and "HW < 2^25" in _err(lib), (HW, Cn, D, S)
    assert lib.goi_codebook_fused_partial_rows() == K["GD_WAVES"]
    assert lib.goi_codebook_dlut_partial_blocks() == K["DLUT_BLOCKS"]


def test_dlut_and_sim_refuse_bad_shapes(lib):
    for HW, Cn, D in ((64, 288, 256), (64, 305, 256), (64, 300, 128), (66, 300, 256)):
        assert lib.goi_codebook_dlut(FAKE, FAKE, HW, Cn, D, FAKE, None) < 0 and "288 < C <= 304" in _err(lib)
    for HW, Cn, D in ((64, 302, 256), (64, 308, 256), (64, 300, 255), (0, 300, 256)):
        rc = lib.goi_codebook_sim(FAKE, FAKE, HW, Cn, D, FAKE, FAKE, FAKE, None)
        assert rc < 0 and "C % 4 = 0" in _err(lib), (HW, Cn, D)
