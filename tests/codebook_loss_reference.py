"""Float64 references and result checkers for the fused semantic-loss path of csrc/codebook_loss.hip (goi_codebook_fused:
codebook_split_k, decoder_split_k, decoder_stats_k, codebook_simgrad_k, decoder_gd_k, codebook_dlut2_k), the
three-kernel path's dLUT GEMM (goi_codebook_dlut: codebook_dlut_k) and the split sim GEMM (goi_codebook_sim:
codebook_sim_k).

Shared by tests/test_gpu_codebook_loss.py, which feeds them device results, and tests/test_codebook_loss_cpu.py, which
feeds them deliberately wrong results and checks the reference against autograd.  The per-pixel mathematics is the row
pass's (semantic_head_reference.loss_terms); only the inputs and the error model differ.  Everything is torch: a check
runs in float64 on the device of its inputs, in pixel chunks.

Reference.  From the kernels' own inputs (g [256, HW], l1 [C, 256], sem [S, HW], W [C, S], b, t): raw = g^T l1^T and
1 / |g| in float64, xs = raw / |g|, z = f W^T + b.  Duplicate code-book rows (bit-identical rows of l1) give
bit-identical products on the kernel, so the reference gives every member of a duplicate group the value of its first
member: the label set is then exactly {c : raw_c = max raw}, arg_s its first member, arg_a the first maximum of z.
The fixtures keep every other decision out of the error band (make_fused_inputs).

Error model (u = 2^-24; every bound is per element and scaled by that element's own terms).
  * Split products.  x = hi + lo + e with hi = rne_bf16(x), lo = rne_bf16(x - hi) (x - hi is exact): |x - hi| <= 2^-8 |x|,
    |lo| <= 2^-8 |x| (1 + 2^-8), |e| <= 2^-16 |x|.  hi*hi + lo*hi + hi*lo is exact in fp32 (8 x 8 bits) and differs from
    a*b by lo_a lo_b + e_a b + a e_b:  |.| <= SP |a||b|,  SP = (3 + 2^-6) 2^-16.
  * MFMA accumulation, modelled as a tree over the K products of one instruction (log2 K roundings) followed by one
    rounding into the accumulator, each of ONE ulp (2u) of its operands' |terms|, not half an ulp: the fp32 16x16x4 MFMA
    is measured ~3 u off on a single dominant product, which round-to-nearest cannot give.  n chained instructions of
    depth d cost 2 (n + d) u of the sum of |terms|.  sim: 8 K chunks x 3 products of K = 32:
    Es_c = (SP + 58 u) sum_k |g_k l_ck| (abs. error of raw_c; codebook_sim_k and codebook_simgrad_k alike).  Logits: the
    bias seeds the accumulator, three products of K = 16:  E_c = SP A_c + 14 u (A_c + |b_c|),  A_c = sum_s |W_cs f_s|.
  * 1 / |g|: 64 fmaf per lane and two shuffle adds (66 u of |g|^2), a correctly rounded sqrtf and division:
    r_inv = 35 u relative.
  * prob_at (decoder_gd_k: P at a label code).  hi + lo of W is exact in fp32 and within 2^-16 |W| of W; one product, a
    16-lane row_sum (4 roundings) and the bias:  E'_c = 2^-16 A_c + 6 u (A_c + |b_c|).  This, not the MFMA logit, enters Pl.
  * P_c = __expf(z_c - mz) / Z.  The shift by mz cancels in exact arithmetic; what is left is, to first order,
        r1_c = E_c + sum_c' P_c' E_c' + ee_c + sum_c' P_c' ee_c' + (NCB + 6) u,   ee_c = u (2 |z_c - max z| + 3)
    (the subtraction and the log2(e) scaling round by u |x| each, v_exp_f32 is one ulp; Z is 19 lane adds + 4 DPP steps,
    then a reciprocal and a multiply), and rP_c = r1_c (1 + 2 r1_c) covers the second order.  rPl_c: E'_c in place of E_c.
  * P2 (decoder_stats_k, fmaf chain + row_sum, times rZ twice):  tP2 = sum 2 P_c^2 rP_c + (NCB + 7) u P2.
    Pl:  tPl = sum_label P_c rPl_c + nl u Pl.
  * dz_c = kappa P_c (P_c - lab_c - P2 + Pl):  t_dz_c = kappa P_c [rP_c (|P_c - lab_c - P2 + Pl| + P_c) + tP2 + tPl
    + 6 u (|P_c - lab_c| + P2 + Pl)]  (kappa's own rounding, two subtractions, three products).
  * dsem_s = sum_c dz_c W_cs: split dz (transposition tile) against the split decoder, three accumulators of 10 K steps of
    32 codes, summed at the end:  t_dsem_s = sum_c |W_cs| t_dz_c + (SP + 32 u) sum_c |dz_c W_cs|.
  * dW_cs of a decoder_gd_k wave over its nb blocks (3 products of K = 16 per block):
        sum_p |f_sp| t_dz_pc + (SP + 2 (3 nb + 4) u) sum_p |dz_pc f_sp|;   db (plain fp32 adds): (nb + 4) u in place of SP + ...
  * exp(t (sim - m)) is exp2(raw tl + nb) with tl = t log2(e) / |g| (3 roundings + r_inv) and nb = -mraw tl folded in.
    With e2_c = t log2(e) (xs_c - m) <= 0 and mt = t log2(e) |m|, the argument's abs. error (log2 units) is
        de2_c = u (mt + 2 |e2_c|) + |e2_c| (3 u + r_inv) + t log2(e) (Es_c + Es_arg_s) / |g|
    and q_c's relative error rq_c = ln2 de2_c + 2 u.  Zq: rZ = sum qh rq + (NCB + 4) u.  k2 = -sum qh e2 (A2 / Zq):
        dk2 = sum qh (de2 + |e2| (rq + rZ + (NCB + 6) u)) + u |k2|,
    H = ln2 (log2 Zq + k2).  The sim errors (eps_c = t Es_c / |g|) enter H through dH/dx_c = -t qh_c (ln qh_c + H) only: a
    shift of every x_c (the error of m) cancels.  With w = sum qh |ln qh + H| the second order is below eps^2 (2 + 2 w):
        t_H = sum qh |ln qh + H| eps + max(eps)^2 (2 + 2 w) + rZ' + ln2 (2 u (log2 Zq + 1) + dk2') + 3 u H
    where rZ', dk2' are rZ, dk2 with the rounding part of de2 alone (v_log_f32: one ulp and 2^-23 absolute).
  * dsim (internal: the dsim planes feed codebook_dlut2_k) = c1 q (e2 + k2) + wone mu with c1 = -g_ent ln2 rZq inv:
        t_dsim_c = inv (g_ent qh_c (|ln qh_c + H| (rZ + r_inv + 11 u + rq_c) + ln2 (de2_c + dk2 + u (|e2_c| + |k2|)))
                   + ind_c / HW (r_inv + 3 u)) + u |dsim_c|
    (g_ent = 0.3 t / HW rounds 4 times, c1 5 more; the fmaf that adds the one-element terms once).
  * dLUT of a codebook_dlut2_k workgroup over its nch 32-pixel chunks (split dsim planes x split g, 3 products of K = 32):
        sum_p |g_dp| t_dsim_pc + (SP + 2 (3 nch + 5) u) sum_p |dsim_pc g_dp|.
    codebook_dlut_k (fp32 MFMA 16x16x4: a rounded product, two tree levels and the accumulator, 8 instructions per 32-pixel
    stage, nst stages, inputs exact):  (16 nst + 6) u sum_p |dsim_pc g_dp|.
  * Loss sums: ms = mraw / |g|: |g|^-1 Es_arg_s + |ms| (r_inv + u); sim_a alike at arg_a; lab term P2 - 2 Pl + nl:
    tP2 + 2 tPl + 3 u (P2 + 2 Pl + nl).  Summation: lab per lane over 4 nb pixels then 6 DPP levels ((4 nb + 6) u); the
    others 4 rows + 6 levels in codebook_simgrad_k, then nb lane adds + 6 levels in decoder_gd_k ((nb + 16) u).
Each checker returns its worst error as a fraction of the bound.  A worst case of 1e-2 .. 1e-1 is expected of the
split-product terms: the bound adds the worst case of 256 (sim), 16 (logits) or 300 (dsem) products whose actual
errors have either sign and cancel like a random walk.  The loss sums m and sim_a add one such sim error per pixel of a
wave (16 nb of them), which cancel once more: ~1e-2 of their bound.
"""
from __future__ import annotations

import math
import re

import torch

from tests import semantic_head_reference as R
from tests.semantic_head_reference import U, _cmp

SP = (3 + 2.0 ** -6) * 2.0 ** -16  # one split-bf16 product (three partial products), relative to |a||b|
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
R_INV = 35 * U


def fused_constants() -> dict:
    """The fused path's tiling, grids and limits, parsed from the source (so that retuning one moves the tests)."""
    cl = R._src("codebook_loss.hip")

    def one(pat, what):
        m = re.search(pat, cl)
        assert m, what + " not found"
        return m

    c = {}
    m = one(r"constexpr int SIM_NCB = (\d+), SIM_NC = SIM_NCB \* 16, SIM_K = (\d+), SIM_KC = (\d+);", "SIM_NCB")
    c["NCB"], c["D"], c["SIM_KC"] = int(m.group(1)), int(m.group(2)), int(m.group(3))
    c["NC"] = 16 * c["NCB"]
    pb = int(one(r"#define GOI_SIM_PB (\d+)", "GOI_SIM_PB").group(1))
    nw = int(one(r"#define GOI_SIM_NW (\d+)", "GOI_SIM_NW").group(1))
    assert "constexpr int SIM_WG_PIX = 16 * SIM_PB * SIM_NW;" in cl
    c["SIM_WG_PIX"] = 16 * pb * nw
    c["DL_KP"] = int(one(r"constexpr int DL_KP = (\d+);", "DL_KP").group(1))
    c["FU_WG_PIX"] = int(one(r"constexpr int FU_WG_PIX = (\d+);", "FU_WG_PIX").group(1))
    c["BLOCK"] = int(one(r"return \(HW \+ FU_WG_PIX - 1\) / FU_WG_PIX \* \(FU_WG_PIX / (\d+)\);", "fu_blocks").group(1))
    c["FU_TIE_WORDS"] = int(one(r"constexpr int FU_TIE_WORDS = (\d+);", "FU_TIE_WORDS").group(1))
    c["FU_NJ"] = (c["NCB"] + 1) // 2
    assert "constexpr int FU_NJ = (SIM_NCB + 1) / 2;" in cl
    c["GD_NW"] = int(one(r"constexpr int GD_NW = (\d+);", "GD_NW").group(1))
    c["DS_NW"] = int(one(r"constexpr int DS_NW = (\d+);", "DS_NW").group(1))
    c["DLUT_BLOCKS"] = int(one(r"int codebook_dlut_blocks\(\) \{ return (\d+); \}", "codebook_dlut_blocks").group(1))
    c["GD_WAVES"] = int(one(r"int codebook_fused_rows\(\) \{ return (\d+) \* GD_NW; \}", "codebook_fused_rows").group(1)) \
        * c["GD_NW"]
    assert "decoder_gd_k<<<dim3(codebook_fused_rows() / GD_NW)" in cl
    m = one(r"decoder_stats_k<<<dim3\(\(unsigned\)\(stat_wgs < (\d+) \? stat_wgs : (\d+)\)\)", "decoder_stats_k grid")
    assert m.group(1) == m.group(2)
    c["DS_WAVES"] = int(m.group(1)) * c["DS_NW"]
    m = one(r"const long long n_chunks = \(HW \+ (\d+)\) / (\d+);  // \2 pixels", "codebook_dlut2_k chunks")
    assert int(m.group(1)) + 1 == int(m.group(2))
    c["DL2_PIX"] = int(m.group(2))
    assert "codebook_dlut2_k<<<dim3(codebook_dlut_blocks())" in cl
    assert "codebook_dlut_k<NCB><<<dim3(2 * codebook_dlut_blocks())" in cl
    m = one(r"C > SIM_NC \|\| C <= SIM_NC - (\d+) \|\| S < 1 \|\| S > (\d+) \|\| HW < (\d+) \|\| \(HW & 3\) != 0 \|\| "
            r"HW >= \(1ll << (\d+)\)\) return -1;", "launch_codebook_fused's shape predicate")
    c["C_MIN"], c["S_MAX"], c["HW_MIN"], c["HW_LIMIT"] = c["NC"] - int(m.group(1)) + 1, int(m.group(2)), int(m.group(3)), \
        1 << int(m.group(4))
    return c


# ---- pixel-to-worker mappings --------------------------------------------------------------------------------------
def fused_blocks(HW: int, K: dict) -> int:
    """16-pixel blocks of the fused path's records (whole codebook_simgrad_k workgroups)."""
    return -(-HW // K["FU_WG_PIX"]) * (K["FU_WG_PIX"] // K["BLOCK"])


def gd_blocks_per_wave(HW: int, K: dict) -> torch.Tensor:
    """[GD_WAVES] blocks each decoder_gd_k wave visits (block i -> wave i mod GD_WAVES)."""
    n, w = fused_blocks(HW, K), torch.arange(K["GD_WAVES"])
    return torch.where(w < n, (n - w + K["GD_WAVES"] - 1) // K["GD_WAVES"], torch.zeros_like(w))


def dlut2_ranges(HW: int, K: dict):
    """codebook_dlut2_k: workgroup b owns 32-pixel chunks [b per, (b + 1) per).  Returns (pixels per workgroup, [(p0, p1)])."""
    n_chunks = -(-HW // K["DL2_PIX"])
    per = -(-n_chunks // K["DLUT_BLOCKS"])
    blen = K["DL2_PIX"] * per
    return blen, [(min(HW, b * blen), min(HW, (b + 1) * blen)) for b in range(K["DLUT_BLOCKS"])]


def dlut_ranges(HW: int, K: dict):
    """codebook_dlut_k: range r owns pixels [r per, (r + 1) per), per = ceil(ceil(HW / ranges) / DL_KP) DL_KP."""
    nr = K["DLUT_BLOCKS"]
    per = -(-(-(-HW // nr)) // K["DL_KP"]) * K["DL_KP"]
    return per, [(min(HW, r * per), min(HW, (r + 1) * per)) for r in range(nr)]


def sim_tolerance_factor(K: dict) -> float:
    """Es_c / sum_k |g_k l_ck|: one split product, and 3 x (K / 32) chained MFMAs of depth 5 at one ulp per rounding."""
    return SP + 2 * (3 * K["D"] // K["SIM_KC"] + 5) * U


def first_duplicate_rows(l1: torch.Tensor) -> torch.Tensor:
    """[C] the lowest code whose code-book row is bit-identical to code c's."""
    return R.first_duplicate(l1, torch.zeros(l1.shape[0], device=l1.device))


# ---- the per-pixel reference and its tolerances ----------------------------------------------------------------------
def fused_pixels(g, l1, first, sem, W, b, t: float, HW_total: int, K: dict) -> dict:
    """Float64 reference and tolerances of a pixel range [m] of the fused path (g [D, m], sem [S, m])."""
    C = l1.shape[0]
    NCB = K["NCB"]
    dev = g.device
    g64 = g.double().T                                    # [m, D]
    L = l1.double()
    raw = (g64 @ L.T)[:, first]                           # duplicates share their first member's value exactly
    graw = (g64.abs() @ L.abs().T)[:, first]
    inv = (g64 * g64).sum(1).rsqrt()
    xs = raw * inv[:, None]
    lab = (raw == raw.amax(1, keepdim=True)).double()
    f = sem.double().T                                    # [m, S]
    W64 = W.double()
    b64 = b.double() if b is not None else torch.zeros(C, dtype=torch.float64, device=dev)
    z = b64[None, :] + f @ W64.T
    A = f.abs() @ W64.abs().T
    r = R.loss_terms(xs, lab, z, t, HW_total, C)
    P, P2, Pl, nl, H, qh = r["P"], r["P2"], r["Pl"], r["nl"], r["H"], r["q"]
    kappa, arg_s, arg_a = r["kappa"], r["arg_s"], r["arg_a"]
    # ---- decoder side
    E = SP * A + 14 * U * (A + b64.abs())
    Ep = 2.0 ** -16 * A + 6 * U * (A + b64.abs())
    ee = U * (2 * (z - z.amax(1, keepdim=True)).abs() + 3)
    common = (P * E).sum(1, keepdim=True) + ee + (P * ee).sum(1, keepdim=True) + (NCB + 6) * U
    r1, r1l = E + common, Ep + common
    rP, rPl = r1 * (1 + 2 * r1), r1l * (1 + 2 * r1l)
    tP2 = (2 * P * P * rP).sum(1) + (NCB + 7) * U * P2
    tPl = (lab * P * rPl).sum(1) + nl * U * Pl
    core = P - lab - P2[:, None] + Pl[:, None]
    t_dz = kappa * P * (rP * (core.abs() + P) + (tP2 + tPl)[:, None]
                        + 6 * U * ((P - lab).abs() + (P2 + Pl)[:, None]))
    dz = r["dz"]
    dsem = dz @ W64
    t_dsem = t_dz @ W64.abs() + (SP + (2 * (K["FU_NJ"] + 5) + 2) * U) * (dz.abs() @ W64.abs())
    # ---- code-book side
    Es = sim_tolerance_factor(K) * graw
    Es_s = Es.gather(1, arg_s[:, None])[:, 0]
    Es_a = Es.gather(1, arg_a[:, None])[:, 0]
    ms, sim_a = r["ms"], r["sim_a"]
    t_ms = inv * Es_s + ms.abs() * (R_INV + U)
    t_sa = inv * Es_a + sim_a.abs() * (R_INV + U)
    tl = t * LOG2E
    e2 = tl * (xs - ms[:, None])
    k2 = -(qh * e2).sum(1)
    g_ent, lnq_H = 0.3 * t / HW_total, r["lq"] + H[:, None]

    def exp_chain(de2):  # relative error of q, of Zq and abs. error of k2 for an argument error de2
        rq = LN2 * de2 + 2 * U
        rZ = (qh * rq).sum(1) + (NCB + 4) * U
        return rq, rZ, (qh * (de2 + e2.abs() * (rq + rZ[:, None] + (NCB + 6) * U))).sum(1) + U * k2.abs()

    de2r = U * (tl * ms.abs()[:, None] + 2 * e2.abs()) + e2.abs() * (3 * U + R_INV)   # the kernel's roundings
    de2 = de2r + tl * inv[:, None] * (Es + Es_s[:, None])                              # and the errors of sim
    rq, rZ, dk2 = exp_chain(de2)
    _, rZr, dk2r = exp_chain(de2r)
    log2Z = torch.logsumexp(e2 * LN2, 1) * LOG2E
    eps = t * inv[:, None] * Es
    sens = qh * lnq_H.abs()
    t_H = (sens * eps).sum(1) + eps.amax(1) ** 2 * (2 + 2 * sens.sum(1)) + rZr + LN2 * (2 * U * (log2Z + 1) + dk2r) \
        + 3 * U * H
    dsim = r["d"] * inv[:, None]
    t_dsim = inv[:, None] * (g_ent * qh * (lnq_H.abs() * (rZ[:, None] + R_INV + 11 * U + rq)
                                           + LN2 * (de2 + dk2[:, None] + U * (e2.abs() + k2.abs()[:, None])))
                             + r["inv_hw"] * r["ind"] * (R_INV + 3 * U)) + U * dsim.abs()
    t_lab = tP2 + 2 * tPl + 3 * U * (P2 + 2 * Pl + nl)
    return dict(dz=dz, t_dz=t_dz, dsem=dsem, t_dsem=t_dsem, dsim=dsim, t_dsim=t_dsim, f=f, lab=lab, arg_s=arg_s,
                arg_a=arg_a, inv=inv, loss=torch.stack([P2 - 2 * Pl + nl, ms, H, sim_a], 1),
                t_loss=torch.stack([t_lab, t_ms, t_H, t_sa], 1))


def row_width(C: int, S: int) -> int:
    return R.row_width(C, S)


def fused_reference(g, l1, sem, W, b, t: float, K: dict, chunk_px: int = 1 << 16) -> dict:
    """Float64 outputs of one goi_codebook_fused call and their tolerances:
    dsem [S, HW]; partials [GD_WAVES, C (S + 1) + 4] (waves without pixels: exact zeros); dlut [n, C, D] for the n
    codebook_dlut2_k workgroups that own pixels (the others, and rows C.. of every workgroup, must be exact zeros)."""
    S, HW = sem.shape
    C, D = l1.shape
    dev = g.device
    first = first_duplicate_rows(l1)
    nW, width, nd = K["GD_WAVES"], row_width(C, S), C * (S + 1)
    blen, ranges = dlut2_ranges(HW, K)
    n_dl = -(-HW // blen)
    chunk = max(1, chunk_px // blen) * blen               # whole dlut2 workgroups, hence whole 16-pixel blocks
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(dsem=torch.zeros(S, HW, **f64), t_dsem=torch.zeros(S, HW, **f64))
    acc, tacc, absacc = (torch.zeros(nW, width, **f64) for _ in range(3))
    dl, tdl, adl = (torch.zeros(n_dl, C, D, **f64) for _ in range(3))
    BLK = K["BLOCK"]
    for p0 in range(0, HW, chunk):
        p1 = min(HW, p0 + chunk)
        m = p1 - p0
        r = fused_pixels(g[:, p0:p1], l1, first, sem[:, p0:p1], W, b, t, HW, K)
        out["dsem"][:, p0:p1] = r["dsem"].T
        out["t_dsem"][:, p0:p1] = r["t_dsem"].T

        def blocks(x, n):
            return torch.nn.functional.pad(x, (0, 0, 0, -(-m // n) * n - m)).view(-1, n, x.shape[1])

        f1 = blocks(torch.cat([r["f"], torch.ones(m, 1, **f64)], 1), BLK)
        dz, t_dz = blocks(r["dz"], BLK), blocks(r["t_dz"], BLK)
        nb = f1.shape[0]
        contrib = torch.cat([torch.bmm(dz.transpose(1, 2), f1).reshape(nb, -1), blocks(r["loss"], BLK).sum(1)], 1)
        tcontrib = torch.cat([torch.bmm(t_dz.transpose(1, 2), f1.abs()).reshape(nb, -1),
                              blocks(r["t_loss"], BLK).sum(1)], 1)
        abscontrib = torch.cat([torch.bmm(dz.abs().transpose(1, 2), f1.abs()).reshape(nb, -1),
                                blocks(r["loss"].abs(), BLK).sum(1)], 1)
        wave = torch.arange(p0 // BLK, p0 // BLK + nb, device=dev) % nW
        acc.index_add_(0, wave, contrib)
        tacc.index_add_(0, wave, tcontrib)
        absacc.index_add_(0, wave, abscontrib)
        # dL/dl1 per codebook_dlut2_k workgroup
        gT = blocks(g[:, p0:p1].double().T, blen)
        ds, tds = blocks(r["dsim"], blen), blocks(r["t_dsim"], blen)
        b0 = p0 // blen
        b1 = b0 + gT.shape[0]
        dl[b0:b1] = torch.bmm(ds.transpose(1, 2), gT)
        tdl[b0:b1] = torch.bmm(tds.transpose(1, 2), gT.abs())
        adl[b0:b1] = torch.bmm(ds.abs().transpose(1, 2), gT.abs())
    nbw = gd_blocks_per_wave(HW, K).to(dev).double()[:, None]
    tol = tacc.clone()
    tol[:, :nd].view(nW, C, S + 1)[:, :, :S] += ((SP + 2 * (3 * nbw + 4) * U)[:, :, None]
                                                 * absacc[:, :nd].view(nW, C, S + 1)[:, :, :S])
    tol[:, :nd].view(nW, C, S + 1)[:, :, S] += (nbw + 4) * U * absacc[:, :nd].view(nW, C, S + 1)[:, :, S]
    tol[:, nd:nd + 1] += (4 * nbw + 6) * U * absacc[:, nd:nd + 1]
    tol[:, nd + 1:] += (nbw + 16) * U * absacc[:, nd + 1:]
    nch = torch.tensor([-(-(q1 - q0) // K["DL2_PIX"]) for q0, q1 in ranges[:n_dl]], **f64)[:, None, None]
    out.update(partials=acc, t_partials=tol, dlut=dl, t_dlut=tdl + (SP + 2 * (3 * nch + 5) * U) * adl)
    return out


LOSS_NAMES = ("lab", "m", "H", "sim_a")


def fused_check(g, l1, sem, W, b, t: float, dsem, partials, dlut, K: dict, chunk_px: int = 1 << 16) -> dict:
    """Checks one goi_codebook_fused call element by element: dsem [S, HW], partials [GD_WAVES, C (S + 1) + 4] and the
    dlut partials [DLUT_BLOCKS, NC, D] (every workgroup; rows C.. and workgroups without pixels exactly zero).  Returns the
    largest error of each output as a fraction of its tolerance."""
    S, HW = sem.shape
    C, D = l1.shape
    ref = fused_reference(g, l1, sem, W, b, t, K, chunk_px)
    nd = C * (S + 1)
    assert partials.shape == (K["GD_WAVES"], nd + 4) and dlut.shape == (K["DLUT_BLOCKS"], K["NC"], D)
    worst = {"dsem": _cmp("dsem", dsem, ref["dsem"], ref["t_dsem"])}
    pw, rw, tw = (x[:, :nd].reshape(-1, C, S + 1) for x in (partials, ref["partials"], ref["t_partials"]))
    worst["dW"] = _cmp("partials (dW)", pw[:, :, :S], rw[:, :, :S], tw[:, :, :S])
    worst["db"] = _cmp("partials (db)", pw[:, :, S], rw[:, :, S], tw[:, :, S])
    for i, name in enumerate(LOSS_NAMES):
        worst[name] = _cmp(f"partials (loss sum {name})", partials[:, nd + i], ref["partials"][:, nd + i],
                           ref["t_partials"][:, nd + i])
    n = ref["dlut"].shape[0]
    worst["dlut"] = _cmp("dlut partials", dlut[:n, :C], ref["dlut"], ref["t_dlut"])
    _zero("dlut partials (padded code rows)", dlut[:, C:])
    _zero("dlut partials (workgroups without pixels)", dlut[n:])
    return worst


def _zero(name, x):
    z = torch.zeros_like(x, dtype=torch.float64)
    _cmp(name, x, z, z)


# ---- codebook_dlut_k and codebook_sim_k ----------------------------------------------------------------------------
def dlut_reference(dsim, g, K: dict, chunk_px: int = 1 << 16):
    """float64 (value, tolerance) [n, C, D] of goi_codebook_dlut's partials for the n ranges that own pixels."""
    HW, C = dsim.shape
    D = g.shape[0]
    per, ranges = dlut_ranges(HW, K)
    n = -(-HW // per)
    f64 = dict(dtype=torch.float64, device=dsim.device)
    val, absv = torch.zeros(n, C, D, **f64), torch.zeros(n, C, D, **f64)
    chunk = max(1, chunk_px // per) * per
    for p0 in range(0, HW, chunk):
        p1 = min(HW, p0 + chunk)
        pad = -(-(p1 - p0) // per) * per - (p1 - p0)
        ds = torch.nn.functional.pad(dsim[p0:p1].double(), (0, 0, 0, pad)).view(-1, per, C)
        gT = torch.nn.functional.pad(g[:, p0:p1].double().T, (0, 0, 0, pad)).view(-1, per, D)
        b0 = p0 // per
        val[b0:b0 + ds.shape[0]] = torch.bmm(ds.transpose(1, 2), gT)
        absv[b0:b0 + ds.shape[0]] = torch.bmm(ds.abs().transpose(1, 2), gT.abs())
    nst = torch.tensor([-(-(q1 - q0) // K["DL_KP"]) for q0, q1 in ranges[:n]], **f64)[:, None, None]
    return val, (16 * nst + 6) * U * absv


def dlut_check(dsim, g, partial, K: dict) -> float:
    """Every range of goi_codebook_dlut against float64; rows C.. and ranges without pixels exactly zero."""
    HW, C = dsim.shape
    val, tol = dlut_reference(dsim, g, K)
    n = val.shape[0]
    assert partial.shape == (K["DLUT_BLOCKS"], K["NC"], g.shape[0])
    worst = _cmp("dlut ranges", partial[:n, :C], val, tol)
    _zero("dlut ranges (padded code rows)", partial[:, C:])
    _zero("dlut ranges (ranges without pixels)", partial[n:])
    return worst


def sim_check(g, l1, sim, inv_gnorm, K: dict, chunk_px: int = 1 << 16):
    """goi_codebook_sim: sim_raw [HW, C] and inv_gnorm [HW] element by element.  Returns (worst sim, worst inv_gnorm)."""
    HW = g.shape[1]
    L = l1.double()
    ws = wi = 0.0
    for p0 in range(0, HW, chunk_px):
        g64 = g[:, p0:p0 + chunk_px].double().T
        raw = g64 @ L.T
        tol = sim_tolerance_factor(K) * (g64.abs() @ L.abs().T)
        ws = max(ws, _cmp("sim_raw", sim[p0:p0 + chunk_px], raw, tol, f" (pixels {p0}..)"))
        inv = (g64 * g64).sum(1).rsqrt()
        wi = max(wi, _cmp("inv_gnorm", inv_gnorm[p0:p0 + chunk_px], inv, R_INV * inv, f" (pixels {p0}..)"))
    return ws, wi


# ---- fixtures ----------------------------------------------------------------------------------------------------------
def tie_groups(C: int):
    """Duplicate code-book rows: two lanes of one 16-code block, the same lane of two blocks, across the tie mask's word
    boundary, on the partly padded last block, and 3-way ties."""
    last = (288, C - 1) if C - 1 > 288 else (150, 288)
    return [(3, 9), (40, 56), (31, 32), last, (100, 101, 200), (64, 127, 250)]


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _draw_g(n, l1, gen, groups):
    """[D, n] ground-truth pixels: a scaled code-book row plus noise (a clear maximum), in a quarter of the pixels noise
    only (close runners-up); with tie groups two thirds of the row pixels pick a duplicated code; magnitudes 2^-3 .. 2^3."""
    C, D = l1.shape
    dev = l1.device
    code = torch.randint(0, C, (n,), generator=gen, device=dev)
    if groups:
        members = torch.tensor([c for grp in groups for c in grp], device=dev)
        pick = members[torch.randint(0, len(members), (n,), generator=gen, device=dev)]
        code = torch.where(torch.rand(n, generator=gen, device=dev) < 2 / 3, pick, code)
    a = 0.5 + 1.5 * torch.rand(n, generator=gen, device=dev)
    a = torch.where(torch.rand(n, generator=gen, device=dev) < 0.25, torch.zeros_like(a), a)
    v = l1[code] * a[:, None] + 0.07 * torch.randn(n, D, generator=gen, device=dev)
    scale = torch.exp2(torch.randint(-3, 4, (n,), generator=gen, device=dev).float())
    return (v * scale[:, None]).T.contiguous().float()


def _draw_sem(S, n, gen, dev, general):
    if general:
        return torch.randn(S, n, generator=gen, device=dev)
    return torch.randint(-32, 33, (S, n), generator=gen, device=dev).float() / 16


def near_ties(g, l1, first, sem, W, b, general: bool, K: dict, chunk_px: int = 1 << 16) -> torch.Tensor:
    """[HW] bool: pixels whose float64 top-two gap of raw sim (between duplicate groups) or, for a general decoder, of z is
    within twice the sum of the two codes' error bounds."""
    HW = g.shape[1]
    L = l1.double()
    C = L.shape[0]
    out = torch.zeros(HW, dtype=torch.bool, device=g.device)
    Esf = sim_tolerance_factor(K)
    for p0 in range(0, HW, chunk_px):
        g64 = g[:, p0:p0 + chunk_px].double().T
        raw = (g64 @ L.T)[:, first]
        Es = Esf * (g64.abs() @ L.abs().T)[:, first]
        top = raw.argmax(1, keepdim=True)
        other = first[None, :] != first[top]
        r2 = torch.where(other, raw, torch.full_like(raw, -math.inf))
        sec = r2.argmax(1, keepdim=True)
        gap = raw.gather(1, top) - raw.gather(1, sec)
        near = (gap <= 2 * (Es.gather(1, top) + Es.gather(1, sec)))[:, 0]
        if general:
            f = sem[:, p0:p0 + chunk_px].double().T
            b64 = b.double() if b is not None else torch.zeros(C, dtype=torch.float64, device=g.device)
            z = b64 + f @ W.double().T
            A = f.abs() @ W.double().abs().T
            E = SP * A + 7 * U * (A + b64.abs())
            v, i = z.topk(2, 1)
            near |= (v[:, 0] - v[:, 1]) <= 2 * (E.gather(1, i[:, :1]) + E.gather(1, i[:, 1:]))[:, 0]
        out[p0:p0 + chunk_px] = near
    return out


def make_fused_inputs(HW: int, C: int, S: int, bias: bool, seed: int, decoder: str = "dyadic", ties: bool = False,
                      device="cpu", K: dict | None = None) -> dict:
    """Inputs of goi_codebook_fused whose discrete decisions are out of the error band.
      decoder "dyadic": W k/8, b k/128, f k/16 (every logit exact, so the argmax of P is exact; W's lo plane is zero) with
        duplicate decoder rows (exact logit ties: arg_a is the first);
      decoder "general": fp32 normal W, f, b: exercises the lo planes; pixels near a logit tie are redrawn.
    ties: duplicate code-book rows (tie_groups) that win most pixels.  Pixels whose sim maximum is within twice its error
    bound of the runner-up are redrawn; the number redrawn is returned as "redrawn" and must be small."""
    K = K or fused_constants()
    dev = torch.device(device)
    gen = _gen(dev, seed)
    D = K["D"]
    l1 = torch.randn(C, D, generator=gen, device=dev)
    l1 = (l1 / l1.norm(dim=1, keepdim=True)).float()
    groups = tie_groups(C) if ties else []
    for grp in groups:
        l1[list(grp[1:])] = l1[grp[0]].clone()
    general = decoder == "general"
    if general:
        W = torch.randn(C, S, generator=gen, device=dev)
        b = 0.5 * torch.randn(C, generator=gen, device=dev) if bias else None
    else:
        W = torch.randint(-8, 9, (C, S), generator=gen, device=dev).float() / 8
        b = torch.randint(-128, 129, (C,), generator=gen, device=dev).float() / 128 if bias else None
        for i in range(0, C - 1, 7):  # duplicate decoder rows (and biases): exact logit ties
            j = int(torch.randint(0, C, (1,), generator=gen, device=dev))
            W[j] = W[i].clone()
            if b is not None:
                b[j] = b[i].clone()
    g = _draw_g(HW, l1, gen, groups)
    sem = _draw_sem(S, HW, gen, dev, general)
    first = first_duplicate_rows(l1)
    redrawn = 0
    for _ in range(20):
        near = near_ties(g, l1, first, sem, W, b, general, K).nonzero()[:, 0]
        if near.numel() == 0:
            break
        redrawn += near.numel()
        g[:, near] = _draw_g(near.numel(), l1, gen, groups)
        sem[:, near] = _draw_sem(S, near.numel(), gen, dev, general)
    else:
        raise AssertionError("near ties left after 20 redraws")
    return dict(g=g, l1=l1.contiguous(), sem=sem.contiguous(), W=W.contiguous(), b=b, redrawn=redrawn)
