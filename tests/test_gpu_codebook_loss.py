"""The fused semantic-loss kernels and the dLUT / sim GEMMs of csrc/codebook_loss.hip called directly through the C ABI,
against the float64 references of tests/codebook_loss_reference.py, element by element.

goi_codebook_fused: every code count 289 .. 304 (S rotating through 1 .. 16, bias on and off, t = 1 and 2, dyadic and
general decoders), every loop edge of the persistent kernels (the 16-pixel block, the 128-pixel workgroup, one trip of
codebook_dlut2_k, decoder_gd_k and decoder_stats_k and one block past it, ~300 000 pixels where every persistent kernel
takes several trips, and the 1600x1056 headline), exact code-book ties at a multi-trip size.  goi_codebook_dlut: every
range at stage and range edges.  goi_codebook_sim: code and workgroup edges.  Exact properties (bit for bit): scaling g
by 2^k, and a zero decoder column.  Refusals leave the outputs untouched.  Every output starts as NaN with one extra
tail element; tests/test_codebook_loss_cpu.py checks that the tables here straddle the bounds parsed from the sources.
"""
from __future__ import annotations

import ctypes as C
import time
import zlib

import pytest
import torch

from tests import codebook_loss_reference as CR

pytestmark = pytest.mark.gpu

K = CR.fused_constants()
WORST = {}  # largest error seen as a fraction of its bound, per output (printed at the end of the module)
HEADLINE = 1600 * 1056

FUSED_C = tuple(range(K["C_MIN"], K["NC"] + 1))
FUSED_HW = (4, 12, 16, 20, 124, 128, 132, 8192, 8196, 32768, 32772, 131072, 131076, 300_004, HEADLINE)
TIES_HW = 32772          # code-book ties where decoder_gd_k takes a second trip
DLUT_C = (289, 292, 300, 303, 304)
DLUT_HW = (4, 28, 32, 36, 8192, 8196, 300_004, HEADLINE)
SIM_C = (4, 16, 64, 300, 304)
SIM_HW = (1, 127, 128, 129, 255, 257, 5000)
SCALE_K = (-20, 7, 20)
REFUSE_HW = 1 << 25


def _lib():
    from goi_hyperplane_amd import _lib as L
    return L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _seed(tag) -> int:
    return zlib.crc32(repr(tag).encode())


def _note(prefix, worst: dict):
    for k, v in worst.items():
        WORST[f"{prefix} {k}"] = max(WORST.get(f"{prefix} {k}", 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    for k in sorted(WORST):
        print(f"worst error / bound {k}: {WORST[k]:.4f}")
    print(f"test_gpu_codebook_loss wall time: {time.time() - t0:.1f} s")


def _nan(n, dev):
    return torch.full((n + 1,), float("nan"), device=dev)


def fused(inp, t):
    """One goi_codebook_fused call on NaN-filled outputs with a tail element; returns (rc, dsem, partials, dlut)."""
    lib = _lib().load()
    g, l1, sem, W, b = (inp[k] for k in ("g", "l1", "sem", "W", "b"))
    S, HW = sem.shape
    Cn, D = l1.shape
    dev = g.device
    nW, NB = lib.goi_codebook_fused_partial_rows(), lib.goi_codebook_dlut_partial_blocks()
    assert nW == K["GD_WAVES"] and NB == K["DLUT_BLOCKS"]
    width = CR.row_width(Cn, S)
    dsem, part, dl = _nan(S * HW, dev), _nan(nW * width, dev), _nan(NB * K["NC"] * D, dev)
    ws = torch.empty((int(lib.goi_codebook_fused_workspace_bytes(HW)),), dtype=torch.uint8, device=dev)
    rc = lib.goi_codebook_fused(_ptr(g), _ptr(l1), _ptr(sem), _ptr(W), _ptr(b), HW, Cn, D, S, float(t), _ptr(dsem),
                                _ptr(part), _ptr(dl), _ptr(ws), None)
    torch.cuda.synchronize()
    for name, x in (("dsem", dsem), ("partials", part), ("dlut", dl)):
        assert torch.isnan(x[-1]), f"{name}: write past the end"
    return rc, dsem[:-1].view(S, HW), part[:-1].view(nW, width), dl[:-1].view(NB, K["NC"], D)


def check_fused(HW, Cn, S, bias, t, decoder, ties=False, seed=None):
    inp = CR.make_fused_inputs(HW, Cn, S, bias, _seed((HW, Cn, S, bias, t, decoder, ties)) if seed is None else seed,
                               decoder=decoder, ties=ties, device="cuda", K=K)
    assert inp["redrawn"] <= HW // 20 + 8, inp["redrawn"]
    rc, dsem, part, dl = fused(inp, t)
    assert rc == 0, _lib().last_error()
    worst = CR.fused_check(inp["g"], inp["l1"], inp["sem"], inp["W"], inp["b"], t, dsem, part, dl, K)
    _note(f"fused ({decoder})", worst)
    return inp, (dsem, part, dl)


# ---- goi_codebook_fused ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", FUSED_C)
def test_fused_every_code_count(Cn):
    """Each C of the last, partly padded code block; S rotates through 1 .. 16 (every 4-channel group edge), bias and t
    alternate; both decoder families at a ragged size (two 128-pixel workgroups and one 4-pixel tail)."""
    i = FUSED_C.index(Cn)
    S = i % 16 + 1
    check_fused(260, Cn, S, bias=i % 2 == 0, t=1.0 + (i // 2) % 2, decoder="dyadic", ties=i % 3 == 0)
    check_fused(260, Cn, 17 - S, bias=i % 2 == 1, t=2.0 - (i // 2) % 2, decoder="general")


@pytest.mark.parametrize("HW", FUSED_HW)
def test_fused_every_loop_edge(HW):
    """The 16-pixel block, the 128-pixel workgroup, one trip of codebook_dlut2_k (256 x 32 pixels), decoder_gd_k
    (2048 waves x 16) and decoder_stats_k (8192 waves x 16) and one block past each; ~300 000 pixels (several trips of
    every persistent kernel) and the headline frame, element by element."""
    i = FUSED_HW.index(HW)
    Cn = FUSED_C[(5 * i) % len(FUSED_C)]
    S = (16, 1, 9, 16, 4)[i % 5]
    check_fused(HW, Cn, S, bias=i % 2 == 0, t=1.0 + i % 2, decoder=("general", "dyadic")[i % 2])


def test_fused_code_book_ties_over_several_trips():
    """Duplicate code-book rows (one block, same lane of two blocks, across the tie-mask word boundary, on the padded
    last block, 2- and 3-way) winning most pixels, where decoder_gd_k and codebook_dlut2_k take a second trip."""
    for Cn, decoder in ((300, "dyadic"), (289, "general"), (304, "general")):
        inp, _ = check_fused(TIES_HW, Cn, 16 if decoder == "dyadic" else 7, True, 2.0, decoder, ties=True)
        raw = inp["g"].double().T @ inp["l1"].double().T
        nl = (raw == raw.amax(1, keepdim=True)).sum(1)
        assert (nl == 2).sum() > TIES_HW // 10 and (nl == 3).sum() > TIES_HW // 10  # the fixture reaches the tie path


def _fused_outputs(inp, t):
    rc, dsem, part, dl = fused(inp, t)
    assert rc == 0, _lib().last_error()
    return dsem.clone(), part.clone(), dl.clone()


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("decoder", ["dyadic", "general"])
def test_fused_scaling_g_by_a_power_of_two_is_exact(decoder):
    """g -> 2^k g: every split, product, sum, sqrtf and reciprocal scales exactly (away from overflow and underflow), so
    dsem, the partial rows and the dlut partials (dsim scales by 2^-k, g by 2^k) are bit-identical."""
    inp = CR.make_fused_inputs(40_004, 297, 11, True, _seed(("scale", decoder)), decoder=decoder, ties=True, device="cuda",
                               K=K)
    base = _fused_outputs(inp, 2.0)
    for k in SCALE_K:
        scaled = dict(inp, g=inp["g"] * 2.0 ** k)
        for name, a, b in zip(("dsem", "partials", "dlut"), base, _fused_outputs(scaled, 2.0)):
            assert torch.equal(_bits(a), _bits(b)), (k, name, int((_bits(a) != _bits(b)).sum()))


@pytest.mark.parametrize("S", [3, 15])
def test_fused_zero_decoder_column_is_invisible(S):
    """S + 1 channels whose extra W column is zero (the extra feature is arbitrary): the first S channels of dsem, dW, db,
    the loss sums and dLUT are bit-identical to the S-channel call."""
    HW, Cn = 33_004, 301
    for decoder in ("dyadic", "general"):
        inp = CR.make_fused_inputs(HW, Cn, S, True, _seed(("zero", S, decoder)), decoder=decoder, device="cuda", K=K)
        gen = torch.Generator(device="cuda").manual_seed(S)
        wide = dict(inp, sem=torch.cat([inp["sem"], 3 * torch.randn(1, HW, device="cuda", generator=gen)]).contiguous(),
                    W=torch.cat([inp["W"], torch.zeros(Cn, 1, device="cuda")], 1).contiguous())
        d0, p0, l0 = _fused_outputs(inp, 1.0)
        d1, p1, l1 = _fused_outputs(wide, 1.0)
        nd0, nd1 = Cn * (S + 1), Cn * (S + 2)
        r0, r1 = p0[:, :nd0].view(-1, Cn, S + 1), p1[:, :nd1].view(-1, Cn, S + 2)
        assert torch.equal(_bits(d0), _bits(d1[:S]))
        assert torch.equal(_bits(r0[:, :, :S]), _bits(r1[:, :, :S]))              # dW
        assert torch.equal(_bits(r0[:, :, S]), _bits(r1[:, :, S + 1]))            # db
        assert torch.equal(_bits(p0[:, nd0:]), _bits(p1[:, nd1:]))                # loss sums
        assert torch.equal(_bits(l0), _bits(l1))
        # the zero column's own gradient, sum_p dz f_S, is not zero: checked against float64 on the wide call
        CR.fused_check(wide["g"], wide["l1"], wide["sem"], wide["W"], wide["b"], 1.0, d1, p1, l1, K)


# ---- goi_codebook_dlut -----------------------------------------------------------------------------------------------
def dlut(dsim, g, Cn, HW, D=256):
    lib = _lib().load()
    NB = lib.goi_codebook_dlut_partial_blocks()
    out = _nan(NB * K["NC"] * 256, dsim.device)
    rc = lib.goi_codebook_dlut(_ptr(dsim), _ptr(g), HW, Cn, D, _ptr(out), None)
    torch.cuda.synchronize()
    assert torch.isnan(out[-1]), "write past the end"
    return rc, out[:-1].view(NB, K["NC"], 256)


def _dsim_like(HW, Cn, seed):
    """dL/dsim_raw-like values: ~1 / HW with a few one-element terms, of both signs, over magnitudes 2^-6 .. 2^6."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(HW, Cn, device="cuda", generator=gen) * torch.exp2(torch.randint(-6, 7, (HW, Cn), device="cuda",
                                                                                   generator=gen).float())
    return (x / max(HW, 1)).contiguous()


@pytest.mark.parametrize("HW", DLUT_HW)
def test_dlut_every_range(HW):
    """Every range of codebook_dlut_k: one stage (HW <= 256 x 32), ragged last stage, several stages (the double-buffered
    stage loop), ranges without pixels (exact zeros), rows C .. 303 exact zeros."""
    cs = DLUT_C if HW <= 8196 else DLUT_C[HW % len(DLUT_C)::3]
    for Cn in cs:
        gen = torch.Generator(device="cuda").manual_seed(_seed((HW, Cn, "g")))
        g = torch.randn(256, HW, device="cuda", generator=gen)
        dsim = _dsim_like(HW, Cn, _seed((HW, Cn)))
        rc, part = dlut(dsim, g, Cn, HW)
        assert rc == 0, _lib().last_error()
        WORST["dlut_k"] = max(WORST.get("dlut_k", 0.0), CR.dlut_check(dsim, g, part, K))


# ---- goi_codebook_sim ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", SIM_C)
def test_sim_element_by_element(Cn):
    lib = _lib().load()
    for HW in SIM_HW:
        gen = torch.Generator(device="cuda").manual_seed(_seed((HW, Cn, "sim")))
        l1 = torch.randn(Cn, 256, device="cuda", generator=gen)
        l1 = (l1 / l1.norm(dim=1, keepdim=True)).contiguous()
        g = (torch.randn(256, HW, device="cuda", generator=gen)
             * torch.exp2(torch.randint(-3, 4, (1, HW), device="cuda", generator=gen).float())).contiguous()
        sim, inv = _nan(HW * Cn, g.device), _nan(HW, g.device)
        ws = torch.empty((int(lib.goi_codebook_sim_workspace_bytes()),), dtype=torch.uint8, device="cuda")
        rc = lib.goi_codebook_sim(_ptr(g), _ptr(l1), HW, Cn, 256, _ptr(sim), _ptr(inv), _ptr(ws), None)
        torch.cuda.synchronize()
        assert rc == 0, _lib().last_error()
        assert torch.isnan(sim[-1]) and torch.isnan(inv[-1]), "write past the end"
        ws_, wi_ = CR.sim_check(g, l1, sim[:-1].view(HW, Cn), inv[:-1], K)
        _note("sim_k", {"sim_raw": ws_, "inv_gnorm": wi_})


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    lib = _lib().load()
    dev = torch.device("cuda")
    small = torch.zeros(1 << 16, device=dev)
    out = torch.full((1 << 16,), float("nan"), device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    rc = lib.goi_codebook_fused(_ptr(small), _ptr(small), _ptr(small), _ptr(small), None, REFUSE_HW, 300, 256, 16, 1.0,
                                _ptr(out), _ptr(out), _ptr(out), _ptr(ws), None)
    torch.cuda.synchronize()
    assert rc < 0 and "HW < 2^25" in _lib().last_error()
    assert torch.isnan(out).all()
    for Cn, D, HW in ((288, 256, 64), (305, 256, 64), (300, 128, 64), (300, 256, 66)):
        rc = lib.goi_codebook_dlut(_ptr(small), _ptr(small), HW, Cn, D, _ptr(out), None)
        torch.cuda.synchronize()
        assert rc < 0 and "288 < C <= 304" in _lib().last_error(), (Cn, D, HW)
        assert torch.isnan(out).all(), (Cn, D, HW)
