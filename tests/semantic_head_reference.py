"""Plain float64 references and result checkers for the semantic head: the inference decode (csrc/semantic_head.hip,
goi_semantic_decode) and the training row pass (csrc/codebook_loss.hip: codebook_rows_k, goi_codebook_loss_rows).

Shared by tests/test_gpu_semantic_head.py, which feeds them device results, and tests/test_semantic_head_cpu.py, which
feeds them deliberately wrong results to show that every check can fail.  Everything is torch, so a check runs on the
device of its inputs (float64 on the GPU for the large shapes) or on the CPU.

Decode.  The logits L[p, c] = b[c] + sum_s W[c, s] f[s, p] are formed in float64 from the fp32 inputs.  A kernel's
idx[p] is accepted when L[p, idx[p]] >= max_c L[p, c] - 2 e_p with e_p = gamma * max_c (|b_c| + sum_s |W_cs f_sp|):
if every computed logit is within e_p of the exact one, the computed argmax can lose at most 2 e_p.  gamma per path,
with u = 2^-24 (padded channels and codes contribute exact zeros, so S counts the real channels):
  * semantic_decode3n_k: every fp32 operand is split exactly into three bf16 parts x = h + m + l (|m| <= 2^-8 |x|,
    |l| <= 2^-16 |x|).  Six of the nine part products are formed, exactly (8 x 8 significant bits); the three dropped
    ones (f_m W_l, f_l W_m, f_l W_l) are below 2^-23 of the product.  The bias seeds an fp32 chain of at most 6 S
    additions, each rounding by u of a partial sum no larger than (1 + 2^-6) (|b| + sum |W f|):
        gamma = (6 S + 4) u.
  * semantic_decode_k: the bias seeds an fp32 chain of K4 v_mfma_f32_16x16x4_f32; each of the S real products
    rounds once and each of their additions once:
        gamma = (2 S + 2) u.
A two-term split (h + m) is accurate to only 2^-16 of each operand.  The ladder fixture (ladder_problem) puts the
gap between two codes entirely into the l part of one weight: at k * gamma <= 2^-17 (k = 3 and 4 at S = 1, 2) such a
kernel sees a tie and keeps the lower, worse code, which the rule above refuses (k >= 3 > 2).

Row pass.  Continuous quantities are float64; the discrete decisions follow the kernel's fp32 quantities:
xs = fp32(sim_raw * inv_gnorm) is one IEEE multiply (reproduced exactly by an fp32 tensor multiply), the label set is
{c : xs_c == max xs}, arg_s its first member, arg_a the first argmax of the decoder logits.  The fixtures put the
decoder inputs on a dyadic grid (weights k/8, features k/16, bias k/128), so that every logit, and hence arg_a, is
exact in fp32 as well.  Per pixel, with zs = max_c (|b_c| + sum_s |W_cs f_s|), span_z = max z - min z and
span_s = max xs - min xs (over real codes):
    E_z   = (S + 1) u zs                                       abs. error of a logit (an fmaf chain of S terms)
    rho   = 4 E_z + (4 span_z + 4 t span_s + C + 16) u         rel. error of every P_c and q_c: __expf is one ulp
                                                               after an argument that rounds by u |z - max z|;
                                                               the normalising sums add C u
    lam   = rho (1 + ln C + t span_s)                          abs. error of log q_c and of the entropy H
Element tolerances (each scaled by the element's own terms, never by a tensor maximum; kappa = 100 / (HW C)):
    dz_c      4 rho kappa P_c (P_c + label_c + sum P^2 + sum_label P)
    dsim_c    |inv| (g q_c (2 rho (|log q_c| + H) + 2 lam) + 6 u M_c),  g = 0.3 t / HW,  M_c = |dL/dxs_c|'s terms
              (6 u: the fp32 1/HW and 0.3 t / HW, two subtractions, the product with inv)
    dsem_s    sum_c |W_cs| tol(dz_c) + (C + 8) u sum_c |dz_c W_cs|
    dW_cs     sum_{p of the wave} |f_sp| tol(dz_pc) + (n + 2) u sum |dz_pc f_sp|     (n pixels of the wave; db: f = 1)
    loss sums the per-pixel errors plus (n + 2) u sum |term| (sim at arg_a and max sim are exact per pixel)
"""
from __future__ import annotations

import math
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "goi_hyperplane_amd", "csrc")
U = 2.0 ** -24  # unit roundoff of fp32


def _src(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def kernel_constants() -> dict:
    """The decode's and the row pass's bounds, parsed from the sources (so that retuning one moves the tests)."""
    sh, cl = _src("semantic_head.hip"), _src("codebook_loss.hip")
    c = {}
    m = re.search(r"const size_t lds = \(\(size_t\)4 \* K4 \* ncp \+ ncp\) \* sizeof\(float\);\s*"
                  r"if \(lds > (\d+) \* 1024\) return -1;", sh)
    assert m, "the fp32 kernel's LDS bound not found"
    c["FP32_LDS"] = int(m.group(1)) * 1024
    m = re.search(r"const size_t lds3 = \(size_t\)ncp \* 16 \* 2 \* 3 \+ \(size_t\)ncp \* 4 \* sizeof\(float\);\s*"
                  r"if \(S <= (\d+) && g_options.decode_variant >= 1 && lds3 <= (\d+) \* 1024\)", sh)
    assert m, "the split kernel's LDS bound not found"
    c["SPLIT_S_MAX"], c["SPLIT_LDS"] = int(m.group(1)), int(m.group(2)) * 1024
    m = re.search(r"if \(blocks > (\d+) \* (\d+)\) blocks = \1 \* \2;", sh)
    assert m, "the fp32 kernel's grid cap not found"
    c["GRID_CAP"] = int(m.group(1)) * int(m.group(2))
    m = re.search(r"if \(K4 == (\d+) && ncp == (\d+) \* 16\) \{", sh)
    assert m, "the fixed-block specialisation not found"
    c["FIXED_K4"], c["FIXED_NBLK"] = int(m.group(1)), int(m.group(2))
    assert "GOI_LAUNCH((semantic_decode_k<%d, %d>));" % (c["FIXED_K4"], c["FIXED_NBLK"]) in sh
    m = re.search(r"if \(S < 1 \|\| S > (\d+) \|\| C < 1 \|\| C > (\d+)\) return -1;", cl)
    assert m, "the row pass's size bound not found"
    c["ROW_S_MAX"], c["ROW_C_MAX"] = int(m.group(1)), int(m.group(2))
    m = re.search(r"int codebook_loss_waves\(\) \{ return (\d+) \* (\d+); \}", cl)
    assert m, "codebook_loss_waves() not found"
    c["ROW_WAVES"] = int(m.group(1)) * int(m.group(2))
    # the row pass's instantiations: one per codes-per-lane count, CPL = ceil(C / 64)
    cases = re.findall(r"GOI_CASE\((\d+)\)", cl[cl.index("int launch_codebook_rows"):])
    c["ROW_CPL"] = sorted(int(x) for x in cases)
    m = re.search(r"__launch_bounds__\(CBL_THREADS, \(CPL <= (\d+) \? 2 : 1\)\) void codebook_rows_k", cl)
    assert m, "codebook_rows_k's launch bound not found"
    c["ROW_CPL_2WG"] = int(m.group(1))
    return c


# ---- decode: which kernel, which LDS, which limit ----------------------------------------------------------------------
def ncp(n_codes: int) -> int:
    return (n_codes + 15) // 16 * 16


def split_lds(n_codes: int) -> int:
    return ncp(n_codes) * (16 * 2 * 3 + 4 * 4)  # three bf16 planes of 16 channels + the bias replicated x4


def fp32_lds(S: int, n_codes: int) -> int:
    return (4 * ((S + 3) // 4) * ncp(n_codes) + ncp(n_codes)) * 4


def split_max_codes(c: dict) -> int:
    return c["SPLIT_LDS"] // (16 * 2 * 3 + 4 * 4) // 16 * 16


def max_codes(S: int, c: dict) -> int:
    """The largest code book goi_semantic_decode accepts at S (the fp32 kernel's LDS)."""
    return c["FP32_LDS"] // (4 * (4 * ((S + 3) // 4) + 1)) // 16 * 16


def decode_path(S: int, n_codes: int, variant: int, c: dict):
    """("split", NPB) or ("fp32", K4, NBLK_T); None when the call is refused."""
    if n_codes > max_codes(S, c):
        return None
    if S <= c["SPLIT_S_MAX"] and variant >= 1 and split_lds(n_codes) <= c["SPLIT_LDS"]:
        return ("split", {1: 2, 2: 4}.get(variant, 1))
    k4 = (S + 3) // 4
    if k4 == c["FIXED_K4"] and ncp(n_codes) == 16 * c["FIXED_NBLK"]:
        return ("fp32", k4, c["FIXED_NBLK"])
    return ("fp32", k4, 0)


def gamma(path, S: int) -> float:
    return (6 * S + 4) * U if path[0] == "split" else (2 * S + 2) * U


# ---- decode: reference and checkers -----------------------------------------------------------------------------------
def decode_check(sem: torch.Tensor, W: torch.Tensor, b: torch.Tensor, idx: torch.Tensor, g: float, chunk: int = 1 << 16):
    """Asserts the eps-argmax rule for every pixel; returns max over pixels of (max L - L[idx]) / (2 e_p) (<= 1)."""
    S, HW = sem.shape
    n = W.shape[0]
    idx = idx.to(sem.device).long()
    assert idx.shape == (HW,)
    bad_range = ((idx < 0) | (idx >= n)).nonzero()
    assert bad_range.numel() == 0, f"code index out of [0, {n}) at pixels {bad_range[:8].flatten().tolist()}"
    # identical (W row, bias) pairs give bit-identical logits on any kernel: the lowest such code must win
    first = first_duplicate(W, b)
    dup = (first[idx] != idx).nonzero()
    assert dup.numel() == 0, (f"pixel {int(dup[0])}: code {int(idx[dup[0]])} won over its identical lower twin "
                              f"{int(first[idx[dup[0]]])}; {dup.numel()} pixels")
    W64, b64 = W.double(), b.double()
    worst = 0.0
    for p0 in range(0, HW, chunk):
        f = sem[:, p0:p0 + chunk].double()                              # [S, m]
        L = b64[None, :] + f.T @ W64.T                                   # [m, n]
        scale = (b64.abs()[None, :] + f.abs().T @ W64.abs().T).amax(1)    # [m]
        lmax = L.amax(1)
        got = L.gather(1, idx[p0:p0 + chunk, None])[:, 0]
        loss = lmax - got
        e2 = 2 * g * scale
        bad = (loss > e2).nonzero()[:, 0]
        if bad.numel():
            p = int(bad[0])
            raise AssertionError(f"pixel {p0 + p}: idx {int(idx[p0 + p])} is {float(loss[p]):.3e} below the best logit "
                                 f"(code {int(L[p].argmax())}); allowed 2 e_p = {float(e2[p]):.3e}; {bad.numel()} pixels")
        r = torch.where(e2 > 0, loss / torch.where(e2 > 0, e2, torch.ones_like(e2)), torch.zeros_like(e2))
        worst = max(worst, float(r.max()) if r.numel() else 0.0)
    return worst


def first_duplicate(W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[n] the lowest code whose (W row, bias) is bit-identical to code c's."""
    rows = torch.cat([W.float(), b.float()[:, None]], 1).view(torch.int32).cpu()
    _, inv = torch.unique(rows, dim=0, return_inverse=True)
    first = torch.full((int(inv.max()) + 1,), W.shape[0], dtype=torch.long)
    first = first.scatter_reduce(0, inv, torch.arange(W.shape[0]), reduce="amin")
    return first[inv].to(W.device)


def decode_outputs_check(idx: torch.Tensor, code_score, thresh: float, sim=None, bg=None):
    """sim = code_score[idx] (0 below thresh), bg = score < thresh, bit for bit; score 0 without a table."""
    idx = idx.long()
    score = code_score.float()[idx] if code_score is not None else torch.zeros(idx.shape, device=idx.device)
    want_bg = score < thresh
    want_sim = torch.where(want_bg, torch.zeros_like(score), score)
    if sim is not None:
        same = sim.float().view(torch.int32) == want_sim.view(torch.int32)
        bad = (~same).nonzero()
        assert bad.numel() == 0, f"sim differs at pixels {bad[:8].flatten().tolist()}"
    if bg is not None:
        bad = (bg.to(torch.uint8) != want_bg.to(torch.uint8)).nonzero()
        assert bad.numel() == 0, f"bg differs at pixels {bad[:8].flatten().tolist()}"


# ---- decode: the exact three-way split, for fixtures and for showing what a two-term split would do --------------------
def bf16_rne(x: np.ndarray) -> np.ndarray:
    """Round fp32 to bf16 (nearest, ties to even), returned as fp32."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def split3(x: np.ndarray):
    x = np.asarray(x, np.float32)
    h = bf16_rne(x)
    r1 = (x - h).astype(np.float32)
    m = bf16_rne(r1)
    l = bf16_rne((r1 - m).astype(np.float32))
    return h, m, l


def split_logits(f: np.ndarray, W: np.ndarray, b: np.ndarray, terms: int) -> np.ndarray:
    """Exact float64 value of what a split contraction sums before rounding: terms = 3 the kernel's six part products,
    terms = 2 a two-term split ((f_h + f_m)(W_h + W_m)).  f [S, P], W [n, S], b [n] -> [P, n]."""
    fh, fm, fl = (np.float64(v) for v in split3(f))
    wh, wm, wl = (np.float64(v) for v in split3(W))
    out = b.astype(np.float64)[None, :] + (fh + fm).T @ (wh + wm).T
    if terms == 3:
        out = out + fl.T @ wh.T + fh.T @ wl.T
    return out


W_LADDER = np.float32(1 + 1.5 * 2 ** -9 - 2 ** -17 + 2 ** -23)  # h = 1, m = 1.5 * 2^-9: up to 2^-16 more stays in l


def ladder_problem(S: int, n_codes: int, k: float, g: float, HW: int, seed: int, a: int = 20, b_: int = 7):
    """Codes a and b_ (a > b_) differ only in channel 0, W[a, 0] - W[b_, 0] = delta = 2 k g W[a, 0]; every pixel's
    channel 0 makes L_a - L_b = k e_p exactly up to fp32 rounding of its value.  All terms of a and b_ are positive;
    every other code is -W[a] / 2 (far below, smaller scale).  Returns (sem [S, HW], W [n, S], b [n]) as numpy fp32."""
    assert n_codes > a > b_ >= 0
    rng = np.random.default_rng(seed)
    wa0 = np.float32(W_LADDER * (1 + 2 * k * g))
    wrow = rng.uniform(0.5, 2.0, S).astype(np.float32)
    wrow[0] = wa0
    W = np.tile((-0.5 * wrow).astype(np.float32), (n_codes, 1))
    W[a] = wrow
    W[b_] = wrow
    W[b_, 0] = W_LADDER
    bias = np.full(n_codes, -0.0, np.float32)
    bias[a] = bias[b_] = np.float32(rng.uniform(0.5, 2.0))
    sem = rng.uniform(0.25, 4.0, (S, HW)).astype(np.float32) * np.exp2(rng.integers(-3, 4, (S, HW))).astype(np.float32)
    delta = np.float64(W[a, 0]) - np.float64(W[b_, 0])
    R = np.float64(bias[a]) + (wrow[1:, None].astype(np.float64) * sem[1:].astype(np.float64)).sum(0)
    # delta f = k g (R + W_a0 f)  ->  f = k g R / (delta - k g W_a0)
    sem[0] = (k * g * R / (delta - k * g * np.float64(W[a, 0]))).astype(np.float32)
    return sem, W, bias


def ladder_ratio(sem, W, bias, g, a=20, b_=7) -> np.ndarray:
    """(L_a - L_b) / e_p per pixel, in float64."""
    f = sem.astype(np.float64)
    L = bias.astype(np.float64)[None, :] + f.T @ W.astype(np.float64).T
    scale = (np.abs(bias.astype(np.float64))[None, :] + np.abs(f).T @ np.abs(W.astype(np.float64)).T).max(1)
    return (L[:, a] - L[:, b_]) / (g * scale)


# ---- row pass ---------------------------------------------------------------------------------------------------------
def row_width(C: int, S: int) -> int:
    return C * (S + 1) + 4


def loss_terms(xs, lab, z, t, HW_total, C):
    """The float64 mathematics of the row losses of one pixel range, shared by the row pass and the fused path
    (tests/codebook_loss_reference.py): xs [m, C] the normalised sim, lab [m, C] the label set (0 / 1), z [m, C] the
    decoder logits.  arg_s is the first member of the label set, arg_a the first maximum of z."""
    dev = xs.device
    arg_a = z.argmax(1)                                   # first maximum
    P = torch.softmax(z, 1)
    ms = xs.amax(1, keepdim=True)
    arg_s = (lab * torch.arange(C, 0, -1, device=dev, dtype=torch.float64)).argmax(1)  # first label
    nl = lab.sum(1)
    lx = t * (xs - ms)
    logZq = torch.logsumexp(lx, 1, keepdim=True)
    lq = lx - logZq
    q = lq.exp()
    H = -(q * lq).sum(1)
    P2 = (P * P).sum(1)
    Pl = (P * lab).sum(1)
    kappa = 100.0 / (HW_total * C)
    inv_hw = 1.0 / HW_total
    dz = P * (kappa * (P - lab) - kappa * (P2 - Pl)[:, None])
    ar = torch.arange(C, device=dev)[None, :]
    ind = (ar == arg_s[:, None]).double() + (ar == arg_a[:, None]).double()
    gq = 0.3 * t * inv_hw * q
    d = -gq * (lq + H[:, None]) - inv_hw * ind          # dL/dxs
    sim_a = xs.gather(1, arg_a[:, None])[:, 0]
    return dict(arg_a=arg_a, arg_s=arg_s, P=P, ms=ms[:, 0], nl=nl, lq=lq, q=q, H=H, P2=P2, Pl=Pl, kappa=kappa,
                inv_hw=inv_hw, dz=dz, ind=ind, gq=gq, d=d, sim_a=sim_a)


def _rows_chunk(sim, inv, sem, W, b, t, HW_total, C):
    """Per-pixel float64 reference and tolerances of one pixel range."""
    S = W.shape[1]
    dev = sim.device
    xs32 = sim.float() * inv.float()[:, None]             # the kernel's fp32 xs, exactly
    xs = xs32.double()
    f = sem.double().T                                    # [m, S]
    W64 = W.double()
    b64 = b.double() if b is not None else torch.zeros(C, dtype=torch.float64, device=dev)
    z = b64[None, :] + f @ W64.T
    zs = (b64.abs()[None, :] + f.abs() @ W64.abs().T).amax(1)
    lab = (xs32 == xs32.amax(1, keepdim=True)).double()
    r = loss_terms(xs, lab, z, t, HW_total, C)
    P, ms, nl, lq, q, H, P2, Pl = (r[k] for k in ("P", "ms", "nl", "lq", "q", "H", "P2", "Pl"))
    kappa, inv_hw, dz, ind, gq, d, sim_a = (r[k] for k in ("kappa", "inv_hw", "dz", "ind", "gq", "d", "sim_a"))
    ms = ms[:, None]
    inv64 = inv.double()
    dsim = d * inv64[:, None]
    dsem = dz @ W64                                        # [m, S]
    # tolerances
    E_z = (S + 1) * U * zs
    span_z = (z.amax(1) - z.amin(1))
    span_s = (xs.amax(1) - xs.amin(1))
    rho = 4 * E_z + (4 * span_z + 4 * t * span_s + C + 16) * U
    lam = rho * (1 + math.log(C) + t * span_s)
    t_dz = 4 * rho[:, None] * kappa * P * (P + lab + (P2 + Pl)[:, None])
    M = gq * (lq.abs() + H[:, None]) + inv_hw * ind
    t_dsim = inv64.abs()[:, None] * (gq * (2 * rho[:, None] * (lq.abs() + H[:, None]) + 2 * lam[:, None]) + 6 * U * M)
    t_dsem = t_dz @ W64.abs() + (C + 8) * U * (dz.abs() @ W64.abs())
    lab_term = P2 - 2 * Pl + nl
    t_lab = 4 * rho * (P2 + 2 * Pl) + (C + 8) * U * (P2 + 2 * Pl + nl)
    t_H = 2 * lam + rho * H
    return dict(dz=dz, t_dz=t_dz, dsim=dsim, t_dsim=t_dsim, dsem=dsem, t_dsem=t_dsem, f=f,
                loss=torch.stack([lab_term, ms[:, 0], H, sim_a], 1), t_loss=torch.stack([t_lab, 0 * H, t_H, 0 * H], 1))


def _cmp(name, got, want, tol, where=""):
    got = got.double()
    bad = ~((got - want).abs() <= tol)                   # NaN fails
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{name}{where}: {int(bad.sum())} elements off; first at flat {i}: got {float(got.flatten()[i])!r}, "
                             f"want {float(want.flatten()[i])!r}, tol {float(tol.flatten()[i]):.3e}")
    r = (got - want).abs() / torch.where(tol > 0, tol, torch.ones_like(tol))
    return float(r.max()) if r.numel() else 0.0


def rows_check(sim_raw, inv_gnorm, sem, W, b, t: float, n_waves: int, dsim, dsem, partials, chunk_px: int = 1 << 13):
    """Checks one call of goi_codebook_loss_rows: dsim [HW, C], dsem [S, HW] against float64 element by element, and
    every wave's partial row (dW rows, db, four loss sums) against the float64 sums over that wave's pixels (chunks
    of 64 pixels, chunk i to wave i mod n_waves); waves without pixels must hold exact zeros.  Returns the largest
    error of each output as a fraction of its tolerance."""
    HW, C = sim_raw.shape
    S = W.shape[1]
    dev = sim_raw.device
    width = row_width(C, S)
    assert partials.shape == (n_waves, width)
    acc = torch.zeros(n_waves, width, dtype=torch.float64, device=dev)
    tacc = torch.zeros(n_waves, width, dtype=torch.float64, device=dev)
    absacc = torch.zeros(n_waves, width, dtype=torch.float64, device=dev)
    npx = torch.zeros(n_waves, dtype=torch.float64, device=dev)
    worst = {"dsim": 0.0, "dsem": 0.0, "dW": 0.0, "loss": 0.0}
    chunk_px = max(64, chunk_px // 64 * 64)
    for p0 in range(0, HW, chunk_px):
        p1 = min(HW, p0 + chunk_px)
        r = _rows_chunk(sim_raw[p0:p1], inv_gnorm[p0:p1], sem[:, p0:p1], W, b, t, HW, C)
        worst["dsim"] = max(worst["dsim"], _cmp("dsim", dsim[p0:p1], r["dsim"], r["t_dsim"], f" (pixels {p0}..)"))
        worst["dsem"] = max(worst["dsem"], _cmp("dsem", dsem[:, p0:p1].T, r["dsem"], r["t_dsem"], f" (pixels {p0}..)"))
        # the 64-pixel chunks' contributions to the partial rows: [chunks, C, S + 1] then the four loss sums
        m = p1 - p0
        nch = (m + 63) // 64
        pad = nch * 64 - m

        def chunks(x):
            return torch.nn.functional.pad(x, (0, 0, 0, pad)).view(nch, 64, x.shape[1])

        f1 = chunks(torch.cat([r["f"], torch.ones(m, 1, dtype=torch.float64, device=dev)], 1))
        dz, t_dz = chunks(r["dz"]), chunks(r["t_dz"])
        contrib = torch.cat([torch.bmm(dz.transpose(1, 2), f1).reshape(nch, -1), chunks(r["loss"]).sum(1)], 1)
        tcontrib = torch.cat([torch.bmm(t_dz.transpose(1, 2), f1.abs()).reshape(nch, -1), chunks(r["t_loss"]).sum(1)], 1)
        abscontrib = torch.cat([torch.bmm(dz.abs().transpose(1, 2), f1.abs()).reshape(nch, -1),
                                chunks(r["loss"].abs()).sum(1)], 1)
        wave = (torch.arange(p0 // 64, p0 // 64 + nch, device=dev) % n_waves)
        acc.index_add_(0, wave, contrib)
        tacc.index_add_(0, wave, tcontrib)
        absacc.index_add_(0, wave, abscontrib)
        npx.index_add_(0, wave, torch.full((nch,), 64.0, dtype=torch.float64, device=dev))
    tol = tacc + (npx[:, None] + 2) * U * absacc
    nd = C * (S + 1)
    worst["dW"] = _cmp("partials (dW, db)", partials[:, :nd], acc[:, :nd], tol[:, :nd])
    worst["loss"] = _cmp("partials (loss sums)", partials[:, nd:], acc[:, nd:], tol[:, nd:])
    return worst


def rows_expected(sim_raw, inv_gnorm, sem, W, b, t: float, n_waves: int):
    """float64 (dsim [HW, C], dsem [S, HW], partials [n_waves, width]) of a small call (the checkers' own tests)."""
    HW, C = sim_raw.shape
    r = _rows_chunk(sim_raw, inv_gnorm, sem, W, b, t, HW, C)
    f1 = torch.cat([r["f"], torch.ones(HW, 1, dtype=torch.float64)], 1)
    part = torch.zeros(n_waves, row_width(C, W.shape[1]), dtype=torch.float64)
    contrib = torch.cat([(r["dz"][:, :, None] * f1[:, None, :]).reshape(HW, -1), r["loss"]], 1)
    part.index_add_(0, (torch.arange(HW) // 64) % n_waves, contrib)
    return r["dsim"], r["dsem"].T.contiguous(), part


def make_rows_inputs(HW: int, C: int, S: int, bias: bool, seed: int, device="cpu", label_ties: bool = True,
                     decoder_ties: bool = True):
    """Inputs of the row pass.  Decoder on a dyadic grid (every logit exact in fp32; duplicate rows are exact ties);
    sim_raw = cos * |g| with 2- and 3-way ties of the row maximum in two thirds of the pixels."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    W = torch.randint(-8, 9, (C, S), generator=g).float() / 8
    b = torch.randint(-128, 129, (C,), generator=g).float() / 128 if bias else None
    sem = torch.randint(-32, 33, (S, HW), generator=g).float() / 16
    if decoder_ties and C >= 4:
        for i in range(0, C - 1, 7):   # duplicate rows (and biases): exact ties of the decoder's logits
            j = int(torch.randint(0, C, (1,), generator=g))
            W[j] = W[i]
            if b is not None:
                b[j] = b[i]
    gn = torch.rand(HW, generator=g) * 3 + 0.25
    inv = (1.0 / gn).float()
    sim_raw = ((torch.rand(HW, C, generator=g) * 2 - 1) * gn[:, None]).float()
    if label_ties and C >= 3:  # equal sim_raw values give equal xs (one multiply): 2 maxima in a third, 3 in a third
        kind = torch.arange(HW) % 3
        mx = sim_raw.amax(1)
        cols = torch.stack([torch.randperm(C, generator=g)[:3] for _ in range(min(HW, 1024))])
        cols = cols[torch.arange(HW) % cols.shape[0]]
        rows = torch.arange(HW)
        for j, need in ((0, 1), (1, 1), (2, 2)):
            sel = kind >= need
            sim_raw[rows[sel], cols[sel, j]] = mx[sel]
    out = dict(sim_raw=sim_raw, inv_gnorm=inv, sem=sem.contiguous(), W=W.contiguous(), b=b)
    return {k: (v.to(device) if v is not None else None) for k, v in out.items()}
