"""Semantic head around the rasterizer: the code-book classifier that turns the
rendered S-dim feature into one of `tab_len` codes, the 256-d code book (LUT), the hyperplane
(LinearSVM) score, and the training losses that tie them together.

Mirrors, with the same names / constructor arguments / file formats so that the reference's
checkpoints load unchanged:
    SemanticModel            scene/semantic_model.py:13-63   ({"args", "state_dict"} save format)
    LinearSVM                networks.py:12-67               (x / 0.3438 -> Linear(256, 1), hinge loss, SGD)
    fit_hyperplane           gui/main.py:1673-1763           (the OSH fine-tune against a mask: one HIP kernel)
    select_gaussians         gui/main.py:400-405             (Gaussians of interest)
    select_instances         --                              (the same mask voted into whole objects: instance.py)
    group_points             gui/main.py:1595-1665           (DBSCAN refinement of the selection: cluster.py)
    relevant_cameras         gui/main.py:407-478             (relevant-camera precompute: masks.py on the device)
    evaluate_cameras         gui/main.py:1957-2016           (eval_epoch's IoU / mPA / mP, utils/image_utils.py:59-102)
    view_frame, video_frames gui/main.py:549-604, 1766-1801  (the displayed frame: display.py on the device)
    compute_similarity       gui/main.py:364-386             (inference decode)
    codebook_losses          train.py:142-163                (training losses)

Inference (`compute_similarity`) is the hot part at GUI frame rate: it runs as ONE fused HIP kernel
(csrc/semantic_head.hip: fp32 MFMA contraction + argmax + per-code score lookup) that reads the
rasterizer's [S, H, W] output directly.  The training losses exist twice: `codebook_losses` restates
train.py line by line in PyTorch (the parity reference: ~40 kernels over [HW,300] tensors, 109 ms
and 21 GB at 1600x1056 on MI355X); `fused_codebook_losses` is the product path.  For the reference's shapes (256-d
features, 289..304 codes, S <= 16) that is `goi_codebook_fused`: four hand-written kernels of csrc/codebook_loss.hip,
no [HW, C] fp32 matrix in memory (the similarity and its gradient exist as MFMA tiles and two bf16 planes), ~3.4 ms and
8.6 GB at 1600x1056.  Other shapes take the three-kernel path (similarity kernel or library GEMM, one row kernel, a
split-K MFMA GEMM for dL/dLUT), which is also the cross-check of tests/test_gpu_losses.py; LOSS_PATH_COUNTS says which ran.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, ptr, stream


class FeatureNorm(torch.nn.Module):
    def forward(self, x):
        return x / x.norm(dim=-1, keepdim=True)


class SemanticModel(torch.nn.Module):
    """num_layer x Linear(+ReLU); the reference instantiates it as a single Linear(sem_dim -> tab_len,
    bias=True) (train.py:64)."""

    def __init__(self, dim_in=64, dim_hidden=128, dim_out=40, num_layer=3, device="cuda", use_bias=False, norm=False):
        super().__init__()
        self.dim_in, self.dim_hidden, self.dim_out, self.num_layer, self.device = dim_in, dim_hidden, dim_out, num_layer, device
        self.args = {"dim_in": dim_in, "dim_hidden": dim_hidden, "dim_out": dim_out, "num_layer": num_layer,
                     "device": device, "use_bias": use_bias, "norm": norm}
        layers = []
        for ind in range(num_layer):
            d_in = dim_in if ind == 0 else dim_hidden
            d_out = dim_out if ind == num_layer - 1 else dim_hidden
            layer = torch.nn.Linear(d_in, d_out, device=device, bias=use_bias)
            torch.nn.init.xavier_uniform_(layer.weight.data)
            act = torch.nn.ReLU() if ind < num_layer - 1 else (FeatureNorm() if norm else torch.nn.Identity())
            layers.extend([layer, act])
        self.layers = torch.nn.Sequential(*layers)

    def forward(self, semantic_features):
        return self.layers(semantic_features)

    @staticmethod
    def load(path, map_location=None):
        pth = torch.load(path, map_location=map_location)
        model = SemanticModel(**pth["args"])
        model.load_state_dict(pth["state_dict"])
        return model

    def save(self, path):
        torch.save({"args": self.args, "state_dict": self.state_dict()}, path)


class LinearSVM(torch.nn.Module):
    """The hyperplane of the paper: one Linear(input_dim -> 1) applied to x / 0.3438, trained with hinge loss and plain
    SGD (networks.py:12-59).  `step` is the reference's per-pixel epoch -- it runs wherever torch runs and is the parity
    reference of `fit_hyperplane`, which runs every epoch of the fit in one HIP kernel."""

    def __init__(self, set_bias=0.86, input_dim=256, lr=0.01):
        super().__init__()
        self.linear = torch.nn.Linear(input_dim, 1)
        b = torch.tensor(set_bias)
        torch.nn.init.constant_(self.linear.bias, float(2 - torch.log(b / (1 - b))))
        self.optimizer = torch.optim.SGD(self.parameters(), lr=lr)

    def weight_set(self, weights):
        with torch.no_grad():
            self.linear.weight.copy_(weights)

    @torch.no_grad()
    def eval_forward(self, x, y):
        """IoU of (output > 0) against (y > 0) over the rows of x."""
        self.optimizer.zero_grad()
        output = self.forward(x).squeeze()
        return calculate_iou(y.squeeze() > 0, output > 0)

    def step(self, x, y):
        """One epoch: hinge loss on x [n, D] against y [n] (or [n, 1]) in {0, 1}, backward, SGD step; returns the loss
        (before the step) and the IoU after it."""
        self.optimizer.zero_grad()
        y = y.squeeze()
        output = self.forward(x).squeeze()
        loss = hinge_loss(output, y)
        loss.backward()
        self.optimizer.step()
        with torch.no_grad():
            output = self.forward(x).squeeze()
            iou = calculate_iou(y > 0, output > 0)
        return loss, iou

    def forward(self, x):
        return self.linear(x / 0.3438)


def hinge_loss(outputs, labels):
    """mean(max(0, 1 - o * (2 y - 1))) (networks.py:62-67)."""
    labels = 2 * labels - 1
    return torch.mean(torch.clamp(1 - outputs * labels, min=0))


def calculate_iou(label, pred):
    """|pred & label| / |pred | label| of two boolean masks as a Python float, NaN for an empty union
    (utils/image_utils.py:59-70)."""
    pred_inds = pred == 1
    label_inds = label == 1
    intersection = torch.logical_and(pred_inds, label_inds).sum()
    union = torch.logical_or(pred_inds, label_inds).sum()
    if union == 0:
        return float("nan")
    return float(intersection) / float(max(union, 1))


@torch.no_grad()
def code_scores(lut: torch.Tensor, score_fn) -> torch.Tensor:
    """Everything after the argmax of gui/main.py:364-386 depends on the code only: fold
    LUT[c] -> L2 normalise -> score_fn (LinearSVM + sigmoid, or a VLM similarity) into a table."""
    normed = lut / lut.norm(dim=-1, keepdim=True)
    return score_fn(normed).reshape(-1).float().contiguous()


def svm_score_fn(svm: LinearSVM):
    return lambda feat: svm(feat).squeeze(-1).sigmoid()


@torch.no_grad()
def compute_similarity(sem_chw: torch.Tensor, mlp: SemanticModel, lut: torch.Tensor, score_fn, thresh: float = 0.5,
                       out_bg_mask: torch.Tensor | None = None, return_index: bool = False):
    """Fused decode of a rendered semantic map `sem_chw` [S, H, W] (the rasterizer's output, NOT
    permuted): returns sim[H*W] with background (sim < thresh) zeroed, like the reference's
    compute_similarity(embedding_feature=[HW,S]).  Runs only on the GPU through libgoi_raster.so.

    Shapes (include/goi_raster.h, goi_semantic_decode): 1 <= S <= 32 and 1 <= tab_len <= 16 * floor(10240 /
    (16 * ceil(S / 4) + 4)), i.e. 2400 codes at S = 16 and 1232 at S = 32; a larger code book raises.  S <= 16 with
    tab_len <= 576 decodes on the split-bf16 kernel, everything else on the fp32-MFMA kernel."""
    if mlp.num_layer != 1:
        raise NotImplementedError("the fused decode covers the reference's configuration: one Linear(S -> tab_len)")
    if not sem_chw.is_cuda:
        raise RuntimeError("goi_hyperplane_amd.semantic: tensors must live on a ROCm GPU; there is no CPU fallback")
    lib = _lib.load()
    lin = mlp.layers[0]
    S = int(sem_chw.shape[0])
    HW = int(sem_chw[0].numel())
    dev = sem_chw.device
    n_codes = int(lin.weight.shape[0])
    if lin.weight.shape[1] != S or lut.shape[0] != n_codes:
        raise ValueError("shape mismatch between features, MLP and LUT")
    sem = sem_chw.contiguous().float()
    w = lin.weight.detach().contiguous().float()
    b = (lin.bias.detach() if lin.bias is not None else torch.zeros(n_codes, device=dev)).contiguous().float()
    table = code_scores(lut, score_fn).to(dev)
    sim = torch.empty(HW, dtype=torch.float32, device=dev)
    idx = torch.empty(HW, dtype=torch.int32, device=dev) if return_index else None
    mask = torch.empty(HW, dtype=torch.uint8, device=dev) if out_bg_mask is not None else None
    p = ptr
    with torch.cuda.device(dev):
        check(lib.goi_semantic_decode(p(sem), S, HW, p(w), p(b), n_codes, p(table), float(thresh), p(sim), p(idx), p(mask),
                                      stream(dev)))
    if out_bg_mask is not None:
        out_bg_mask[:] = mask.bool()
    return (sim, idx) if return_index else sim


@torch.no_grad()
def compute_similarity_reference(embedding_feature: torch.Tensor, mlp, lut, score_fn, thresh: float = 0.5,
                                 out_bg_mask=None):
    """The unfused restatement of gui/main.py:364-386 (argmax over softmax(10 * dec), LUT gather,
    normalise, score, threshold) on [HW, S] features.  Used by the tests as the torch reference."""
    dec_feature = mlp(embedding_feature)
    sem_logit = torch.softmax(dec_feature * 10, dim=-1).argmax(dim=-1)
    sem_feature = lut[sem_logit]
    normed_feature = sem_feature / sem_feature.norm(dim=-1, keepdim=True)
    sim = score_fn(normed_feature).reshape(-1)
    bg = sim < thresh
    if out_bg_mask is not None:
        out_bg_mask[:] = bg
    sim = sim.clone()
    sim[bg] = 0
    return sim, sem_logit


def codebook_losses(sem_feature_chw: torch.Tensor, semantic_mlp: SemanticModel, lut: torch.Tensor, gtl_chw: torch.Tensor,
                    iteration: int):
    """Training losses of train.py:142-163.  sem_feature_chw [S,H,W] is the rasterizer output
    (gradients flow back into it), gtl_chw [ape_dim,H,W] the per-view ground-truth APE feature.
    Returns (loss, dict of the four terms)."""
    S = sem_feature_chw.shape[0]
    sem_feature = sem_feature_chw.permute(1, 2, 0).reshape(-1, S)
    sem_label = torch.softmax(semantic_mlp(sem_feature), dim=-1)
    gtl = gtl_chw.permute(1, 2, 0).reshape(-1, gtl_chw.shape[0]).float()
    gtl = gtl / gtl.norm(dim=1, keepdim=True)
    lut1 = lut / lut.norm(dim=1, keepdim=True)
    sim = gtl @ lut1.T  # [HW, tab_len]: the dense code book x feature contraction (library GEMM)
    sim_val = sim.max(dim=1, keepdim=True)[0]
    label = (sim == sim_val).float().detach()
    lab = F.mse_loss(sem_label, label) * 50
    sl = 1 - sim_val.mean()
    recc = 1 - F.cosine_similarity(lut[sem_label.argmax(-1)], gtl, dim=-1).mean()
    t = 1 if iteration < 1000 else 2
    anneal = sim * t
    sl1 = -1.0 * (torch.softmax(anneal, dim=1) * torch.log_softmax(anneal, dim=1)).sum(dim=-1).mean()
    loss = lab + sl + 0.3 * sl1 + recc
    return loss, {"lab": lab, "sl": sl, "sl1": sl1, "recc": recc}


# which implementation the last loss evaluations took, counted (tests assert on it: the product path for the reference's shapes
# is "fused"; "three_kernel" / "library_gemm" are the paths for other shapes)
LOSS_PATH_COUNTS = {"fused": 0, "three_kernel": 0, "library_gemm": 0}
_SIM_KERNEL = {"on": True}  # False: the library fp32 GEMM for sim (A/B and a fallback for other shapes)
_FUSED_KERNELS = {"on": True}  # False: the three-kernel path (sim, rows, dLUT) -- kept for other shapes and as a cross-check


class _FusedCodebookLoss(torch.autograd.Function):
    """loss = lab + sl + 0.3 sl1 + recc of train.py:142-163, with all gradients produced in the forward
    (the loss is a scalar: backward only scales them)."""

    @staticmethod
    def forward(ctx, sem_chw, weight, bias, lut1, gtl_chw, t):
        lib = _lib.load()
        if not sem_chw.is_cuda:
            raise RuntimeError("goi_hyperplane_amd.semantic: tensors must live on a ROCm GPU; there is no CPU fallback")
        dev = sem_chw.device
        S = int(sem_chw.shape[0])
        HW = int(sem_chw[0].numel())
        C, D = int(lut1.shape[0]), int(lut1.shape[1])
        sem = sem_chw.detach().contiguous().float().view(S, HW)
        g = gtl_chw.detach().contiguous().float().view(D, HW)  # [D, HW]: used as g^T through views, never copied
        w = weight.detach().contiguous().float()
        b = None if bias is None else bias.detach().contiguous().float()
        l1 = lut1.detach().contiguous().float()
        with torch.cuda.device(dev):
            p, s = ptr, stream(dev)
            # (the full shape predicate of launch_codebook_fused, csrc/codebook_loss.hip: anything else takes the
            # three-kernel path below instead of raising)
            if (_FUSED_KERNELS["on"] and D == 256 and 288 < C <= 304 and 1 <= S <= 16 and HW % 4 == 0
                    and 4 <= HW < (1 << 25)):
                # sim -> losses -> gradients in two kernels, no [HW, C] fp32 matrix (csrc/codebook_loss.hip: codebook_fused_k)
                dsem = torch.empty((S, HW), dtype=torch.float32, device=dev)
                partials = torch.empty((lib.goi_codebook_fused_partial_rows(), C * (S + 1) + 4), dtype=torch.float32, device=dev)
                part = torch.empty((lib.goi_codebook_dlut_partial_blocks(), 304, D), dtype=torch.float32, device=dev)
                ws = torch.empty((int(lib.goi_codebook_fused_workspace_bytes(HW)),), dtype=torch.uint8, device=dev)
                check(lib.goi_codebook_fused(p(g), p(l1), p(sem), p(w), p(b), HW, C, D, S, float(t), p(dsem), p(partials), p(part),
                                             p(ws), s))
                del ws
                LOSS_PATH_COUNTS["fused"] += 1
                return _FusedCodebookLoss._finish(ctx, sem_chw, bias, partials, dsem, part.sum(dim=0)[:C].contiguous(), HW, C, S)
            sim_raw = inv_gnorm = None
            if D == 256 and C <= 304 and C % 4 == 0 and _SIM_KERNEL["on"]:
                # one pass over g: split-bf16 MFMA contraction + 1/|g| (csrc/codebook_loss.hip: codebook_sim_k)
                sim_raw = torch.empty((HW, C), dtype=torch.float32, device=dev)
                inv_gnorm = torch.empty((HW,), dtype=torch.float32, device=dev)
                ws = torch.empty((int(lib.goi_codebook_sim_workspace_bytes()),), dtype=torch.uint8, device=dev)
                check(lib.goi_codebook_sim(p(g), p(l1), HW, C, D, p(sim_raw), p(inv_gnorm), p(ws), s))
                LOSS_PATH_COUNTS["three_kernel"] += 1
            else:
                LOSS_PATH_COUNTS["library_gemm"] += 1
                inv_gnorm = torch.linalg.vector_norm(g, dim=0).reciprocal_()        # [HW]
                sim_raw = torch.matmul(g.t(), l1.t())                                 # [HW, C]  (library GEMM, fp32)
            dsim = torch.empty_like(sim_raw)
            dsem = torch.empty((S, HW), dtype=torch.float32, device=dev)
            rows = lib.goi_codebook_loss_partial_rows()
            partials = torch.empty((rows, C * (S + 1) + 4), dtype=torch.float32, device=dev)
            check(lib.goi_codebook_loss_rows(p(sim_raw), p(inv_gnorm), p(sem), p(w), p(b), HW, C, S, float(t), p(dsim),
                                             p(dsem), p(partials), s))
            del sim_raw
            if D == 256 and 288 < C <= 304 and HW % 4 == 0:
                # split-K MFMA GEMM over the pixel axis with a persistent [304, 256] accumulator per CU
                blocks = lib.goi_codebook_dlut_partial_blocks()
                part = torch.empty((blocks, 304, D), dtype=torch.float32, device=dev)
                check(lib.goi_codebook_dlut(p(dsim), p(g), HW, C, D, p(part), s))
                dl1 = part.sum(dim=0)[:C].contiguous()
            else:
                dl1 = torch.matmul(dsim.t(), g.t())                                   # [C, D]   (library GEMM)
        return _FusedCodebookLoss._finish(ctx, sem_chw, bias, partials, dsem, dl1, HW, C, S)

    @staticmethod
    def _finish(ctx, sem_chw, bias, partials, dsem, dl1, HW, C, S):
        tot = partials.sum(dim=0)                                                     # fixed order: reproducible
        dWb = tot[: C * (S + 1)].view(C, S + 1)
        sums = tot[C * (S + 1):]
        lab = sums[0] * (50.0 / (HW * C))
        sl = 1.0 - sums[1] / HW
        sl1 = sums[2] / HW
        recc = 1.0 - sums[3] / HW
        ctx.save_for_backward(dsem.view_as(sem_chw), dWb[:, :S].contiguous(), dWb[:, S].contiguous(), dl1)
        ctx.has_bias = bias is not None
        terms = torch.stack([lab, sl, sl1, recc])
        ctx.mark_non_differentiable(terms)
        return lab + sl + 0.3 * sl1 + recc, terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        dsem, dW, db, dl1 = ctx.saved_tensors
        return (grad_loss * dsem, grad_loss * dW, (grad_loss * db) if ctx.has_bias else None, grad_loss * dl1, None, None)


def fused_codebook_losses(sem_feature_chw: torch.Tensor, semantic_mlp: SemanticModel, lut: torch.Tensor,
                          gtl_chw: torch.Tensor, iteration: int):
    """Drop-in for `codebook_losses` (same arguments, same (loss, dict) result, same gradients into the
    rasterizer output, the decoder and the code book) running on the GPU as described in
    csrc/codebook_loss.hip.  Covers the reference's configuration: one Linear(S -> tab_len) decoder,
    S <= 16, tab_len <= 512."""
    if semantic_mlp.num_layer != 1:
        raise NotImplementedError("the fused losses cover the reference's configuration: one Linear(S -> tab_len)")
    lin = semantic_mlp.layers[0]
    lut1 = lut / lut.norm(dim=1, keepdim=True)  # differentiable: the kernel returns dL/dlut1
    t = 1.0 if iteration < 1000 else 2.0
    loss, terms = _FusedCodebookLoss.apply(sem_feature_chw, lin.weight, lin.bias, lut1, gtl_chw, t)
    return loss, {"lab": terms[0], "sl": terms[1], "sl1": terms[2], "recc": terms[3]}


# ---- the optimisable semantic-space hyperplane (OSH) fine-tune: gui/main.py:1673-1763 (finetune_prompt_with_res) ---------
# Every pixel's feature is one of n_codes normalised LUT rows, so the reference's per-pixel loop (hinge loss, SGD, IoU per
# epoch) depends on the frame only through P[c] / N[c], the mask-positive / -negative pixel counts per code.
# csrc/osh.hip counts them in one pass and runs every epoch of the fit, with its stop test, in one workgroup.

OSH_MAX_CODES = 1000
OSH_MAX_DIM = 1024
OSH_MAX_EPOCHS = 1_000_000

OSHFit = namedtuple("OSHFit", ["epochs", "loss", "iou", "init_iou", "trace"])
OSHFit.__doc__ = ("Result of fit_hyperplane: epochs run, the last epoch's loss (before its step), the IoU after the last "
                  "step and that of the initial hyperplane (Python floats; NaN for an empty union), and with return_trace "
                  "a float64 [epochs, 2] tensor of (loss, IoU) per epoch (else None).")

_NO_CPU = "goi_hyperplane_amd.semantic: tensors must live on a ROCm GPU; there is no CPU fallback"


@torch.no_grad()
def osh_counts(idx: torch.Tensor, positive: torch.Tensor, n_codes: int) -> torch.Tensor:
    """int32 [2, n_codes]: row 0 the pixels with idx == c and positive != 0, row 1 those with positive == 0 (one HIP
    kernel over idx [HW] int32 and positive [HW] bool / uint8).  Codes outside [0, n_codes) are not counted."""
    n_codes = int(n_codes)
    if not 1 <= n_codes <= OSH_MAX_CODES:
        raise ValueError(f"osh_counts: n_codes must be in 1..{OSH_MAX_CODES}, got {n_codes}")
    if idx.numel() != positive.numel():
        raise ValueError("osh_counts: idx and positive must have the same number of elements")
    if not (idx.is_cuda and positive.is_cuda):
        raise RuntimeError(_NO_CPU)
    dev = idx.device
    idx = idx.reshape(-1).to(torch.int32).contiguous()
    pos = positive.reshape(-1)
    pos = (pos if pos.dtype == torch.uint8 else (pos != 0).to(torch.uint8)).contiguous()
    counts = torch.zeros((2, n_codes), dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.goi_semantic_osh_counts(ptr(idx), ptr(pos), idx.numel(), n_codes, ptr(counts), stream(dev)))
    return counts


def _osh_launch(lut, counts, HW, w, b, lr, max_epochs, target_iou, return_trace):
    """Launches goi_semantic_osh_fit on copies of w [K, D] / b [K]; returns (w, b, packed result buffer, trace view).
    Nothing is synchronised: the packed buffer holds epochs (int32 [K]), loss (fp32 [K]), iou and init_iou (fp64 [K])."""
    n_codes, D = int(lut.shape[0]), int(lut.shape[1])
    if not 1 <= n_codes <= OSH_MAX_CODES:
        raise ValueError(f"the hyperplane fit covers 1..{OSH_MAX_CODES} codes, got {n_codes}")
    if not 1 <= D <= OSH_MAX_DIM:
        raise ValueError(f"the hyperplane fit covers features of 1..{OSH_MAX_DIM} dimensions, got {D}")
    max_epochs = int(max_epochs)
    if not 1 <= max_epochs <= OSH_MAX_EPOCHS:
        raise ValueError(f"max_epochs must be in 1..{OSH_MAX_EPOCHS}, got {max_epochs}")
    HW = int(HW)
    if not 1 <= HW < 2 ** 31:
        raise ValueError(f"HW must be in 1..2^31-1, got {HW}")
    K = int(w.shape[0])
    if counts.shape != (K, 2, n_codes) or w.shape != (K, D) or b.shape != (K,):
        raise ValueError(f"shapes: counts {tuple(counts.shape)} must be ({K}, 2, {n_codes}), w {tuple(w.shape)} ({K}, {D}), "
                         f"b {tuple(b.shape)} ({K},)")
    if not (lut.is_cuda and counts.is_cuda and w.is_cuda and b.is_cuda):
        raise RuntimeError(_NO_CPU)
    dev = lut.device
    lut = lut.detach().float().contiguous()
    counts = counts.to(torch.int32).contiguous()
    w = w.detach().float().clone().contiguous()
    b = b.detach().float().clone().contiguous()
    buf = torch.empty(24 * K + (16 * K * max_epochs if return_trace else 0), dtype=torch.uint8, device=dev)
    epochs, loss = buf[: 4 * K].view(torch.int32), buf[4 * K: 8 * K].view(torch.float32)
    iou, init_iou = buf[8 * K: 16 * K].view(torch.float64), buf[16 * K: 24 * K].view(torch.float64)
    trace = buf[24 * K:].view(torch.float64).view(K, max_epochs, 2) if return_trace else None
    if trace is not None:
        trace.fill_(float("nan"))
    p = ptr
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.goi_semantic_osh_fit(p(lut), n_codes, D, p(counts), HW, K, p(w), p(b), float(lr), max_epochs,
                                       float(target_iou), p(epochs), p(loss), p(iou), p(init_iou), p(trace), stream(dev)))
    return w, b, buf, trace


def _osh_unpack(buf_cpu, K, max_epochs, return_trace):
    epochs = buf_cpu[: 4 * K].view(torch.int32)
    if (epochs < 0).any():
        raise ValueError("a code present in the frame has an all-zero LUT row (the reference's fit would be NaN)")
    loss = buf_cpu[4 * K: 8 * K].view(torch.float32)
    iou, init_iou = buf_cpu[8 * K: 16 * K].view(torch.float64), buf_cpu[16 * K: 24 * K].view(torch.float64)
    trace = buf_cpu[24 * K: 24 * K + 16 * K * max_epochs].view(torch.float64).view(K, max_epochs, 2) if return_trace else None
    return epochs, loss, iou, init_iou, trace


@torch.no_grad()
def fit_hyperplanes_counts(lut: torch.Tensor, counts: torch.Tensor, HW: int, w: torch.Tensor, b: torch.Tensor, lr: float = 0.01,
                           max_epochs: int = 8000, target_iou: float = 0.9, return_trace: bool = False):
    """K independent hyperplane fits over one code book, all in one launch (one workgroup each): lut [n_codes, D],
    counts [K, 2, n_codes] (osh_counts of each mask), HW the pixels per frame, initial w [K, D] and b [K].  Returns
    (w [K, D], b [K], [OSHFit per fit]) after one device synchronisation; each OSHFit's trace is [epochs, 2] or None."""
    K = int(w.shape[0])
    w, b, buf, _ = _osh_launch(lut, counts, HW, w, b, lr, max_epochs, target_iou, return_trace)
    epochs, loss, iou, init_iou, trace = _osh_unpack(buf.cpu(), K, int(max_epochs), return_trace)
    fits = [OSHFit(int(epochs[i]), float(loss[i]), float(iou[i]), float(init_iou[i]),
                   trace[i, : int(epochs[i])].clone() if return_trace else None) for i in range(K)]
    return w, b, fits


def _decode_idx(sem_chw, mlp, n_codes):
    """argmax code per pixel (goi_semantic_decode's idx_out), int32 [HW]."""
    lin = mlp.layers[0]
    S, HW, dev = int(sem_chw.shape[0]), int(sem_chw[0].numel()), sem_chw.device
    sem = sem_chw.detach().contiguous().float()
    W = lin.weight.detach().contiguous().float()
    bias = (lin.bias.detach() if lin.bias is not None else torch.zeros(n_codes, device=dev)).contiguous().float()
    idx = torch.empty(HW, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().goi_semantic_decode(ptr(sem), S, HW, ptr(W), ptr(bias), n_codes, None, 0.0, None, ptr(idx), None,
                                              stream(dev)))
    return idx


@torch.no_grad()
def fit_hyperplane(sem_chw: torch.Tensor, mlp: SemanticModel, lut: torch.Tensor, positive: torch.Tensor, svm: LinearSVM,
                   max_epochs: int = 8000, target_iou: float = 0.9, return_trace: bool = False) -> OSHFit:
    """The fine-tune of gui/main.py:1673-1763 on the GPU: decode the rendered map sem_chw [S, H, W] to codes, count the
    mask `positive` (H*W elements in sem_chw's pixel order; bool, uint8 or float with values 0 / 1) per code, and fit
    `svm` (hinge loss, SGD with its optimizer's lr) until the IoU is no longer below target_iou or max_epochs have run.
    svm.linear is updated in place.  One device synchronisation, at the end."""
    if mlp.num_layer != 1:
        raise NotImplementedError("the fused decode covers the reference's configuration: one Linear(S -> tab_len)")
    lin = mlp.layers[0]
    n_codes, S = int(lin.weight.shape[0]), int(sem_chw.shape[0])
    if lin.weight.shape[1] != S or lut.shape[0] != n_codes:
        raise ValueError("shape mismatch between features, MLP and LUT")
    if n_codes > OSH_MAX_CODES:
        raise ValueError(f"the hyperplane fit covers up to {OSH_MAX_CODES} codes (the reference slices the decode to "
                         f"[:, :1000]), got {n_codes}")
    HW = int(sem_chw[0].numel())
    if positive.numel() != HW:
        raise ValueError(f"positive has {positive.numel()} elements, the frame {HW} pixels")
    weight, bias = svm.linear.weight, svm.linear.bias
    if weight.shape[1] != lut.shape[1]:
        raise ValueError("LinearSVM input_dim differs from the LUT's feature size")
    if not sem_chw.is_cuda or not positive.is_cuda or not lut.is_cuda:
        raise RuntimeError(_NO_CPU)
    lr = svm.optimizer.param_groups[0]["lr"]
    pos = positive.reshape(-1)
    bad = None if pos.dtype == torch.bool else ((pos != 0) & (pos != 1)).any()
    idx = _decode_idx(sem_chw, mlp, n_codes)
    counts = osh_counts(idx, pos, n_codes)
    w, b, buf, _ = _osh_launch(lut, counts.unsqueeze(0), HW, weight.detach().reshape(1, -1), bias.detach().reshape(1),
                               lr, max_epochs, target_iou, return_trace)
    if bad is not None:
        buf = torch.cat([buf, bad.reshape(1).to(torch.uint8)])
    host = buf.cpu()  # the one synchronisation
    if bad is not None and bool(host[-1]):
        raise ValueError("positive must hold only 0 and 1")
    epochs, loss, iou, init_iou, trace = _osh_unpack(host, 1, int(max_epochs), return_trace)
    weight.copy_(w.reshape(weight.shape))
    bias.copy_(b.reshape(bias.shape))
    n = int(epochs[0])
    return OSHFit(n, float(loss[0]), float(iou[0]), float(init_iou[0]), trace[0, :n].clone() if return_trace else None)


@torch.no_grad()
def select_gaussians(pc, mlp: SemanticModel, lut: torch.Tensor, score_fn, thresh: float = 0.5) -> torch.Tensor:
    """The Gaussians of interest (gui/main.py:400-405, compute_relative_gs_index): the fused decode of every Gaussian's
    own semantic feature pc.get_semantics [P, S], scored by score_fn and thresholded; bool [P], ready for
    render(..., gaussian_mask=...).  (It also returns Gaussians no camera shows: contrib.lift_mask selects by the blend instead.)"""
    sem = pc.get_semantics.detach().float().t().contiguous()  # [S, P]: the decode's channel-major layout, one "pixel" per Gaussian
    return compute_similarity(sem, mlp, lut, score_fn, thresh) > 0


@torch.no_grad()
def select_instances(pc, mlp: SemanticModel, lut: torch.Tensor, score_fn, thresh: float, segments, min_fraction=0.5,
                     min_hits: int = 1, capacity=None) -> torch.Tensor:
    """The OBJECTS of interest: select_gaussians' per-Gaussian prompt mask -- which has holes inside objects and speckle outside
    them -- voted over the instances of `segments` (segment.instances of the same model): an instance is returned whole when at
    least min_hits of its Gaussians and at least min_fraction of them were selected (instance.select).  bool [P], ready for
    render(..., gaussian_mask=..., in_place=True), edit.transform and prune_points.  capacity as in instance.members: None
    reads the number of instances back once, an int synchronises nothing."""
    from . import instance
    return instance.select(segments, select_gaussians(pc, mlp, lut, score_fn, thresh), min_fraction, min_hits, capacity)


@torch.no_grad()
def group_points(pc, selected: torch.Tensor, viewpoint_camera, bg_color: torch.Tensor, mlp: SemanticModel, lut: torch.Tensor,
                 score_fn, res_mask: torch.Tensor, eps: float = 0.35, min_samples: int = 600, keep_ratio: float = 0.7,
                 thresh: float = 0.5, scaling_modifier: float = 1.0, gaussian_mask: torch.Tensor | None = None,
                 in_place: bool = False, mask_invert: bool = False) -> torch.Tensor:
    """The cluster refinement of the retrieved Gaussians (gui/main.py:1595-1665, group_points) on the device.

    `selected` (bool [P], e.g. select_gaussians' result) picks the Gaussians whose positions pc.get_xyz are clustered with
    the exact DBSCAN(eps, min_samples) of cluster.dbscan.  For every cluster, in ascending label order and noise skipped, the
    semantics of all other Gaussians are masked out (pc.set_semantic_masks), the view is rendered with render_gui
    (scaling_modifier, gaussian_mask) and decoded with compute_similarity(thresh); a cluster that shows no semantic pixel is
    dropped (the reference's cos_sim.sum() == 0), and one is kept when |sem & res| / |sem| > keep_ratio, sem = (decoded
    similarity > 0) and res = (res_mask != 0).  That ratio is compute_mask_ratio's elementwise definition
    (utils/image_utils.py:36-48), evaluated as the reference does (fp32 quotient, compared in fp64); res_mask is any tensor
    with H*W elements in the frame's pixel order, as `positive` is in fit_hyperplane (the reference's [1,H,W]-against-[H,W,1]
    comment would broadcast and cannot be meant literally).

    Returns the refined selection, bool [P]: the union of the kept clusters.  Unlike the reference, pc's semantic mask is
    left as it was found and the caller applies the result (gui/main.py:1664 stores it as rel_gs_index).  The ratios are
    accumulated on the device: host synchronisations are the index gather of `selected` and dbscan's one read of the
    cluster count, none per cluster.  With rasterizer.set_geometry_cache on, the K renders of one camera share the
    geometry: renders 2..K are blend-only.  in_place / mask_invert: how gaussian_mask is applied (render.render): handed to
    the rasterizer as a selection instead of index-selecting the model for every cluster's render -- the same result.
    (contrib.lift_mask lifts res_mask, or the masks of several views, onto the Gaussians directly, without clustering.)"""
    from . import cluster
    from .render import render_gui

    P = int(pc.get_xyz.shape[0])
    if selected.numel() != P:
        raise ValueError(f"selected has {selected.numel()} elements, the model {P} Gaussians")
    H, W = int(viewpoint_camera.image_height), int(viewpoint_camera.image_width)
    if res_mask.numel() != H * W:
        raise ValueError(f"res_mask has {res_mask.numel()} elements, the frame {H * W} pixels")
    if not (selected.is_cuda and res_mask.is_cuda and pc.get_xyz.is_cuda):
        raise RuntimeError(_NO_CPU)
    dev = pc.get_xyz.device
    sel_idx = torch.nonzero(selected.reshape(-1)).reshape(-1)
    labels = cluster.dbscan(pc.get_xyz.detach()[sel_idx].float().contiguous(), eps, min_samples)
    K = cluster.dbscan.last_n_clusters
    res = (res_mask.reshape(-1) != 0)
    keep = torch.zeros(K, dtype=torch.bool, device=dev)
    saved = pc._semantics_masks
    try:
        for k in range(K):
            member = torch.zeros(P, dtype=torch.bool, device=dev)
            member.index_put_((sel_idx,), labels == k)
            pc.set_semantic_masks(member)
            out = render_gui(viewpoint_camera, pc, bg_color, scaling_modifier, gaussian_mask=gaussian_mask, in_place=in_place,
                             mask_invert=mask_invert)
            sem = compute_similarity(out["semantics"], mlp, lut, score_fn, thresh).reshape(-1) > 0
            n_sem = sem.sum()
            ratio = (sem & res).sum().float() / n_sem.float()
            keep[k] = (n_sem > 0) & (ratio.double() > keep_ratio)
    finally:
        pc._semantics_masks = saved
    picked = (labels >= 0) & keep[labels.clamp(min=0)] if K else torch.zeros_like(labels, dtype=torch.bool)
    result = torch.zeros(P, dtype=torch.bool, device=dev)
    result.index_put_((sel_idx,), picked)
    return result


RelevantCameras = namedtuple("RelevantCameras", ["index", "counts", "semantic_mask", "semantic_mask_dilated"])
RelevantCameras.__doc__ = ("Result of relevant_cameras: index (list of the kept camera numbers, in camera order), counts "
                           "(int64 [V] on the device: count_nonzero of every camera's decoded similarity, the reference's "
                           "relative_pixel_number), semantic_mask and semantic_mask_dilated (bool [K, 1, H, W], kept cameras "
                           "only, in index order).")

SegEvaluation = namedtuple("SegEvaluation", ["iou", "mpa", "mp", "mean_iou", "mean_mpa", "mean_mp"])
SegEvaluation.__doc__ = ("Result of evaluate_cameras: per-view iou (float64 [V]), mpa and mp (float32 [V]) as CPU tensors, "
                         "and their means (Python floats: iou summed in float64, mpa / mp in float32, each divided by V).")


def _sweep_frame(cameras):
    cams = list(cameras)
    if not cams:
        raise ValueError("the camera set is empty")
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    for i, cam in enumerate(cams):
        if (int(cam.image_height), int(cam.image_width)) != (H, W):
            raise ValueError(f"all cameras must share one frame size: camera 0 is {H}x{W}, camera {i} "
                             f"{int(cam.image_height)}x{int(cam.image_width)}")
    return cams, H, W


def _sweep_pack(cams, H, W, pc, mlp, lut, score_fn, thresh, bg_color, scaling_modifier):
    """Renders and decodes every camera and packs `sim > 0` into slot v of one buffer, with the two counts (masks.pack_into).
    No synchronisation of its own."""
    from . import masks
    from .render import render_gui
    dev = pc.get_xyz.device
    packed = torch.empty((len(cams), H, masks.words(W)), dtype=torch.int64, device=dev)
    counts = torch.zeros((len(cams), 2), dtype=torch.int64, device=dev)
    for v, cam in enumerate(cams):
        out = render_gui(cam, pc, bg_color, scaling_modifier)
        sim = compute_similarity(out["semantics"], mlp, lut, score_fn, thresh)
        masks.pack_into(sim.reshape(H, W), packed, counts, v)
    return packed, counts


def relevant_keep(count: torch.Tensor, min_ratio: float = 0.1) -> torch.Tensor:
    """The camera filter of gui/main.py:470-477 as one tensor expression on the per-camera count_nonzero values (int64
    [V], any device, no synchronisation): kept iff count > 0 (the cos_sim.any() guard of :433) and not
    count < count.max() * min_ratio.  int64 times a Python float is float32, and the comparison is made in float32, as in
    the reference."""
    return (count > 0) & ~(count < count.max() * min_ratio)


@torch.no_grad()
def relevant_cameras(cameras, pc, mlp: SemanticModel, lut: torch.Tensor, score_fn, thresh: float, bg_color: torch.Tensor,
                     kernel_size: int = 3, iterations: int = 5, min_ratio: float = 0.1,
                     scaling_modifier: float = 1.0) -> RelevantCameras:
    """The relevant-camera precompute (gui/main.py:407-478, pre_compute_relative_cameras; gui/main_edit.py:320-394) on the
    device.  With pc's semantic masks cleared (set_semantic_masks() as at :410), every camera in order is rendered with
    render_gui, decoded with compute_similarity(thresh), and its mask cos_sim > 0 and count torch.count_nonzero(cos_sim)
    go into slot v of one packed buffer (masks.pack_into).  After the loop: one batched dilation by
    np.ones((kernel_size, kernel_size)) with `iterations` (the reference's cv2.dilate(...) >= 0.5, masks.dilate), and the
    filter on the device with the reference's expression, so with its dtype promotion (int64 count times a Python float
    is float32): camera v is kept iff count[v] > 0 (the cos_sim.any() guard) and not count[v] < count.max() * min_ratio.
    Then ONE host read-back (the kept flags) and the unpacking of the kept views only.  The renders take whatever forward
    mode is set; the mask stage adds no synchronisation.

    All cameras must share one H x W (ValueError otherwise).  Unlike the reference nothing is written onto the camera
    objects, and pc's semantic mask is restored on exit.  A GUI port attaches the masks itself:
        for k, i in enumerate(res.index):
            cams[i].semantic_mask, cams[i].semantic_mask_dilated = res.semantic_mask[k], res.semantic_mask_dilated[k]
    and keeps relative_cameras = [cams[i] for i in res.index]."""
    from . import masks
    r = masks.radius(kernel_size, iterations)
    cams, H, W = _sweep_frame(cameras)
    if not pc.get_xyz.is_cuda:
        raise RuntimeError(_NO_CPU)
    saved = pc._semantics_masks
    try:
        pc.set_semantic_masks()
        packed, counts = _sweep_pack(cams, H, W, pc, mlp, lut, score_fn, thresh, bg_color, scaling_modifier)
    finally:
        pc._semantics_masks = saved
    dilated = masks.dilate_packed(packed, W, r)
    count = counts[:, 0]
    keep = relevant_keep(count, min_ratio)
    keep_host = keep.cpu()  # the one read-back
    index = torch.nonzero(keep_host).reshape(-1).tolist()
    kept = torch.sort((~keep).to(torch.uint8), stable=True).indices[: len(index)]  # the same indices, on the device
    return RelevantCameras(index, count, masks.unpack(packed, W, kept), masks.unpack(dilated, W, kept))


@torch.no_grad()
def evaluate_cameras(cameras, gt_masks: torch.Tensor, pc, mlp: SemanticModel, lut: torch.Tensor, score_fn, thresh: float,
                     bg_color: torch.Tensor, scaling_modifier: float = 1.0) -> SegEvaluation:
    """The segmentation evaluation of gui/main.py:1957-2016 (eval_epoch) on the device: every camera is rendered with
    render_gui, decoded with compute_similarity(thresh) and its prediction cos_sim > 0 packed; gt_masks ([V, H, W], or
    any CUDA tensor of V*H*W elements in pixel order; positive where != 0) is packed in one launch, one confusion launch
    counts TP / FP / FN / TN per view, and the [V, 4] counts are read back once for masks.segmentation_metrics.  The
    formulas are those of utils/image_utils.py:59-102 on same-shape masks (eval_epoch itself passes a [H, W, C] ground
    truth against a [H, W, 1] prediction, which calculate_mean_pixel_accuracy's shape assert rejects).  The means are the
    sums over the views divided by V, so a NaN view makes its mean NaN, as in eval_epoch.  pc is rendered as it is (the
    reference does not touch its semantic mask here)."""
    from . import masks
    cams, H, W = _sweep_frame(cameras)
    V = len(cams)
    if gt_masks.numel() != V * H * W:
        raise ValueError(f"gt_masks has {gt_masks.numel()} elements, {V} views of {H}x{W} need {V * H * W}")
    if not (gt_masks.is_cuda and pc.get_xyz.is_cuda):
        raise RuntimeError(_NO_CPU)
    gt = gt_masks.reshape(V, H, W)
    if gt.dtype != torch.uint8:
        gt = gt != 0
    pred, _ = _sweep_pack(cams, H, W, pc, mlp, lut, score_fn, thresh, bg_color, scaling_modifier)
    gt_packed = torch.empty_like(pred)
    masks.pack_into(gt, gt_packed)
    m = masks.segmentation_metrics(masks.confusion_packed(pred, gt_packed, W).cpu())
    total_iou, total_mpa, total_mp = 0.0, torch.zeros((), dtype=torch.float32), torch.zeros((), dtype=torch.float32)
    for v in range(V):  # eval_epoch's running sums, in its order and precision
        total_iou += float(m.iou[v])
        total_mpa = total_mpa + m.mpa[v]
        total_mp = total_mp + m.mp[v]
    return SegEvaluation(m.iou, m.mpa, m.mp, total_iou / V, float(total_mpa / V), float(total_mp / V))


# ---- the viewer's frame (gui/main.py:549-604 test_step, :387-398 set_clip_mask, :1766-1801 render_video) -----------------
FRAME_MODES = ("image", "depth", "alpha", "semantics")


class _FrameDecoder:
    """The fused decode with everything that does not depend on the view prepared once (weights, bias, the per-code score
    table): decode(sem_chw, sim_out, mask_out) writes one view's similarity (background zeroed) and its uint8 background
    mask into the caller's buffers.  One launch per view."""

    def __init__(self, mlp, lut, score_fn, thresh, dev):
        if mlp.num_layer != 1:
            raise NotImplementedError("the fused decode covers the reference's configuration: one Linear(S -> tab_len)")
        lin = mlp.layers[0]
        self.n_codes, self.S = int(lin.weight.shape[0]), int(lin.weight.shape[1])
        if lut.shape[0] != self.n_codes:
            raise ValueError("shape mismatch between features, MLP and LUT")
        self.w = lin.weight.detach().contiguous().float()
        self.b = (lin.bias.detach() if lin.bias is not None else torch.zeros(self.n_codes, device=dev)).contiguous().float()
        self.table = code_scores(lut, score_fn).to(dev)
        self.thresh = float(thresh)

    def decode(self, sem_chw, sim_out, mask_out):
        if int(sem_chw.shape[0]) != self.S:
            raise ValueError("shape mismatch between features, MLP and LUT")
        sem = sem_chw.contiguous().float()
        HW = int(sem[0].numel())
        dev = sem.device
        p = ptr
        with torch.cuda.device(dev):
            check(_lib.load().goi_semantic_decode(p(sem), self.S, HW, p(self.w), p(self.b), self.n_codes, p(self.table),
                                                  self.thresh, p(sim_out), None, p(mask_out), stream(dev)))


def _alpha_mask(out, pca_mask_alpha):
    """The samples a frame's own PCA fit uses: alpha > pca_mask_alpha (None: every pixel)."""
    return None if pca_mask_alpha is None else out["alpha"].reshape(-1) > float(pca_mask_alpha)


def _frame_args(mode, style, pc, basis=None, pca_normalize="sigma"):
    from . import display, pca
    if mode not in FRAME_MODES:
        raise ValueError(f"mode must be one of {FRAME_MODES}, got {mode!r}")
    if mode == "semantics":
        if pca_normalize not in pca.NORMALIZATIONS:
            raise ValueError(f"pca_normalize must be one of {sorted(pca.NORMALIZATIONS)}, got {pca_normalize!r}")
        if basis is not None and not isinstance(basis, pca.PcaBasis):
            raise TypeError(f"basis must be a pca.PcaBasis, got {type(basis).__name__}")
    if not pc.get_xyz.is_cuda:
        raise RuntimeError(_NO_CPU)
    return display._style(style)


@torch.no_grad()
def video_frames(cameras, pc, mlp: SemanticModel, lut: torch.Tensor, score_fn, thresh: float, bg_color: torch.Tensor,
                 mode: str = "image", style="heat", overlay_ratio: float = 1.0, gaussian_mask=None,
                 scaling_modifier: float = 1.0, dtype: torch.dtype = torch.uint8, heat_thresh: float = 0.7,
                 colormap: torch.Tensor | None = None, in_place: bool = False, mask_invert: bool = False, basis=None,
                 pca_normalize: str = "sigma", pca_mask_alpha: float | None = None) -> torch.Tensor:
    """The frames of render_video's loop (gui/main.py:1766-1801) for a camera set, [V, H, W, 3] on the device (uint8 as
    the reference saves them, or float32): every camera is rendered with render_gui and decoded with the fused decode
    into slot v of preallocated [V, ...] buffers, then ONE batched display.compose makes all the frames, each view with
    its own minimum and maximum.  `mode` picks the render's "image", "depth" (min-max normalised per view, as
    test_step's depth mode) or "alpha"; `style` is a display style (display.from_reference_flags maps the GUI's
    switches).  Styles that need no similarity skip the decode.  All cameras must share one H x W.  Nothing is read back
    to the host -- with a gaussian_mask only when in_place=True hands it to the rasterizer as a selection (render.render;
    mask_invert: its complement, the viewer's del mode): the default index-select synchronises once per frame.

    mode "semantics" shows the rendered feature map through a PCA basis (pca.py), normalised by `pca_normalize` ("sigma",
    "minmax" or "raw").  With basis=None ONE basis is fitted for the whole camera set, so the colours do not flicker: a
    first sweep renders every view and accumulates its features (those with alpha > pca_mask_alpha, if given) into the
    fit's workspace, keeping no map; the basis is solved on the device and every view is rendered AGAIN to be projected.
    That is two renders per view with flat memory.  Passing a basis (pca.fit_gaussians(pc), say) renders once.
    pca_mask_alpha only selects what a fit made HERE uses: it is ignored when a basis is passed.  In the other modes
    basis, pca_normalize and pca_mask_alpha are neither used nor checked."""
    from . import display
    from .render import render_gui
    code = _frame_args(mode, style, pc, basis, pca_normalize)
    cams, H, W = _sweep_frame(cameras)
    dev = pc.get_xyz.device
    V, HW = len(cams), H * W
    need_sim = code != display.NONE
    semantics = mode == "semantics"
    if semantics:
        from . import pca
        if basis is None:
            fit = pca.Fit(int(pc.get_semantics.shape[1]), dev)
            for cam in cams:
                out = render_gui(cam, pc, bg_color, scaling_modifier, gaussian_mask=gaussian_mask, in_place=in_place,
                                 mask_invert=mask_invert)
                fit.add(out["semantics"], "planar", _alpha_mask(out, pca_mask_alpha))
            basis = fit.solve()
    base = torch.empty((V, 3 if mode in ("image", "semantics") else 1, H, W), dtype=torch.float32, device=dev)
    sim = torch.empty((V, HW), dtype=torch.float32, device=dev) if need_sim else None
    mask = torch.empty((V, HW), dtype=torch.uint8, device=dev) if need_sim else None
    dec = _FrameDecoder(mlp, lut, score_fn, thresh, dev) if need_sim else None
    for v, cam in enumerate(cams):
        out = render_gui(cam, pc, bg_color, scaling_modifier, gaussian_mask=gaussian_mask, in_place=in_place,
                         mask_invert=mask_invert)
        if semantics:
            pca.transform(out["semantics"], basis, normalize=pca_normalize, out=base[v])
        else:
            base[v].copy_(out[mode].reshape(base.shape[1:]))
        if need_sim:
            dec.decode(out["semantics"], sim[v], mask[v])
    return display.compose(base, sim, mask, style=code, normalize=mode == "depth", overlay_ratio=overlay_ratio,
                           heat_thresh=heat_thresh, colormap=colormap, dtype=dtype)


@torch.no_grad()
def view_frame(camera, pc, mlp: SemanticModel, lut: torch.Tensor, score_fn, thresh: float, bg_color: torch.Tensor,
               mode: str = "image", style="heat", overlay_ratio: float = 1.0, gaussian_mask=None,
               scaling_modifier: float = 1.0, dtype: torch.dtype = torch.float32, heat_thresh: float = 0.7,
               colormap: torch.Tensor | None = None, return_parts: bool = False, in_place: bool = False,
               mask_invert: bool = False, basis=None, pca_normalize: str = "sigma", pca_mask_alpha: float | None = None):
    """One displayed frame [H, W, 3] on the device: test_step with set_clip_mask (gui/main.py:549-604, :387-398) as
    render_gui, the fused decode with its uint8 background mask, and display.compose on the render's own tensor (no copy
    of the image).  `mode`, `style` and the rest as video_frames; float32 is what the viewer's texture takes.  Nothing is
    read back to the host (with a gaussian_mask: when in_place=True, see video_frames).  return_parts: also the dictionary
    {"base", "sim", "bg_mask"} the frame was composed from (sim and bg_mask None for the styles that need no similarity).
    mode "semantics": the base is pca.transform(out["semantics"], basis, normalize=pca_normalize); with basis=None the
    basis is fitted on this frame alone (on its pixels with alpha > pca_mask_alpha, if given, so that an empty background
    does not own the first component) -- fit one basis for an orbit and pass it to keep the colours from flickering.
    pca_mask_alpha is ignored when a basis is passed; in the other modes the three PCA arguments are neither used nor
    checked."""
    from . import display
    from .render import render_gui
    code = _frame_args(mode, style, pc, basis, pca_normalize)
    dev = pc.get_xyz.device
    out = render_gui(camera, pc, bg_color, scaling_modifier, gaussian_mask=gaussian_mask, in_place=in_place,
                     mask_invert=mask_invert)
    if mode == "semantics":
        from . import pca
        if basis is None:
            basis = pca.fit(out["semantics"], "planar", _alpha_mask(out, pca_mask_alpha))
        base = pca.transform(out["semantics"], basis, normalize=pca_normalize)
    else:
        base = out[mode]
    base = base.reshape((-1,) + tuple(base.shape[-2:]))
    sim = mask = None
    if code != display.NONE:
        HW = int(base.shape[-2]) * int(base.shape[-1])
        sim = torch.empty(HW, dtype=torch.float32, device=dev)
        mask = torch.empty(HW, dtype=torch.uint8, device=dev)
        _FrameDecoder(mlp, lut, score_fn, thresh, dev).decode(out["semantics"], sim, mask)
    frame = display.compose(base, sim, mask, style=code, normalize=mode == "depth", overlay_ratio=overlay_ratio,
                            heat_thresh=heat_thresh, colormap=colormap, dtype=dtype)
    return (frame, {"base": base, "sim": sim, "bg_mask": mask}) if return_parts else frame


# ---- code-book initialisation (train.py:78-86) -------------------------------------------------------------------------
# How unique_rows moves maps that start on the host: "pageable" is a plain .to(device) per map; "pinned" stages them
# through two reusable pinned buffers, the host copy into one overlapping the DMA out of the other.  Measured on 25 maps
# of 432 MB: pageable 0.282 s, pinned staging 0.293 s for the whole stage, so pageable is the default.
# Maps the caller has pinned already are copied asynchronously either way.
CODEBOOK_STAGING = "pageable"
_STAGING = {}
_CODEBOOK_FLAG_NONFINITE = 1  # GOI_CODEBOOK_FLAG_NONFINITE (include/goi_raster.h)


def _staging_buffers(nbytes):
    bufs = _STAGING.get("bufs")
    if bufs is None or bufs[0].numel() < nbytes:
        bufs = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        _STAGING["bufs"] = bufs
    return bufs


def _maps_to_device(maps, dev):
    """fp32 device copies (or the maps themselves) of [D, H, W] maps on the host or the device."""
    out = [None] * len(maps)
    host = [i for i, m in enumerate(maps) if not m.is_cuda]
    for i, m in enumerate(maps):
        if m.is_cuda:
            out[i] = m.float().contiguous()
    if not host:
        return out
    main = torch.cuda.current_stream(dev)
    staged = [i for i in host if not maps[i].is_pinned()] if CODEBOOK_STAGING == "pinned" else []
    for i in host:
        if i not in staged:
            out[i] = maps[i].to(dev, non_blocking=maps[i].is_pinned())
    if staged:
        nbytes = max(maps[i].numel() * maps[i].element_size() for i in staged)
        bufs = _staging_buffers(nbytes)
        copy = _STAGING.setdefault(("stream", dev), torch.cuda.Stream(dev))
        copy.wait_stream(main)
        done = [None, None]
        for n, i in enumerate(staged):
            m, b = maps[i].contiguous(), n & 1
            if done[b] is not None:
                done[b].synchronize()  # the DMA out of this buffer has finished
            buf = bufs[b][:m.numel() * m.element_size()].view(m.dtype).view(m.shape)
            buf.copy_(m)
            with torch.cuda.stream(copy):
                out[i] = torch.empty(m.shape, dtype=m.dtype, device=dev)
                out[i].copy_(buf, non_blocking=True)
                done[b] = torch.cuda.Event()
                done[b].record(copy)
        main.wait_stream(copy)
        for i in staged:
            out[i].record_stream(main)
    return [o.float().contiguous() for o in out]


@torch.no_grad()
def unique_rows(maps):
    """x.permute(1, 2, 0).reshape(-1, D).unique(dim=0) of each [D, H, W] map (train.py:80), on the device: a list of
    [N_v, D] float32 CUDA tensors (a single map gives a list of one).  Exact: rows are compared by value (-0 == +0) and
    come out in ascending lexicographic order, as torch.unique(dim=0) on the CPU orders them.  Maps may live on the host
    or the device, in float32, float16 or bfloat16 (conversion to float32 is exact and keeps the order).  One read-back
    of the counts of all views of a shape; NaN or Inf in a map raises ValueError (the reference's order is undefined
    there).  Maps on the host are copied per view (CODEBOOK_STAGING)."""
    lst = [maps] if torch.is_tensor(maps) else list(maps)
    if not lst:
        return []
    for m in lst:
        if not torch.is_tensor(m) or m.dim() != 3:
            raise ValueError("unique_rows: every map must be a [D, H, W] tensor")
        if m.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"unique_rows: maps must be float32, float16 or bfloat16, got {m.dtype}")
    dev = next((m.device for m in lst if m.is_cuda), None) or torch.device("cuda", torch.cuda.current_device())
    dmaps = _maps_to_device(lst, dev)
    groups = {}
    for i, m in enumerate(dmaps):
        groups.setdefault(tuple(m.shape), []).append(i)
    lib = _lib.load()
    out = [None] * len(lst)
    for (D, H, W), idx in groups.items():
        V = len(idx)
        ws = torch.empty(max(int(lib.goi_codebook_unique_rows_workspace_bytes(V, D, H, W)), 1), dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * V)(*[dmaps[i].data_ptr() for i in idx])
        counts = (C.c_longlong * V)()
        flags = C.c_uint(0)
        alloc = _lib.TensorAlloc(lambda nbytes: torch.empty(nbytes, dtype=torch.uint8, device=dev))
        with torch.cuda.device(dev):
            r = lib.goi_codebook_unique_rows(ptrs, V, D, H, W, counts, C.byref(flags), alloc.cb, None, ptr(ws), stream(dev))
        check(r, ValueError)
        if alloc.error is not None:
            raise alloc.error
        if flags.value & _CODEBOOK_FLAG_NONFINITE:
            raise ValueError("unique_rows: a map holds NaN or Inf values (the order of unique(dim=0) is undefined there)")
        if flags.value:
            raise RuntimeError(f"unique_rows: device flag word {flags.value:#x} (sort or table bound hit); the rows are not usable")
        rows = alloc.tensor[:sum(counts) * D * 4].view(torch.float32).view(-1, D)
        start = 0
        for j, i in enumerate(idx):
            out[i] = rows[start:start + counts[j]]
            start += counts[j]
    return out


@torch.no_grad()
def spherical_kmeans_batched(xs, ncluster: int, niter: int = 10):
    """io.kmeans (train.py:36-56) of every [N_i, D] float32 CUDA tensor of xs in ONE set of launches: a list of
    [ncluster, D] centres.  Same RNG draws as calling io.kmeans on each in list order (torch.randperm(N_i) on the CPU
    default generator, 1 + niter times each, drawn up front), same in-place normalisation of every x, RuntimeError where
    the reference raises (more dead centres than rows; the generator is then left as the reference leaves it).  fp32
    arithmetic, deterministic means (bit-reproducible); the argmax can differ from a library matmul only at near-ties."""
    xs = list(xs)
    if not xs:
        return []
    ncluster, niter = int(ncluster), int(niter)
    if ncluster < 1:
        raise ValueError("spherical_kmeans: ncluster must be >= 1")
    if niter < 0:
        raise ValueError("spherical_kmeans: niter must be >= 0")
    D = int(xs[0].shape[1]) if xs[0].dim() == 2 else -1
    for x in xs:
        if not torch.is_tensor(x) or x.dim() != 2 or int(x.shape[1]) != D:
            raise ValueError("spherical_kmeans: every x must be [N, D] with the same D")
        if x.dtype != torch.float32:
            raise TypeError(f"spherical_kmeans: x must be float32, got {x.dtype}")
        if not x.is_cuda:
            raise RuntimeError(_NO_CPU)
    sizes = [int(x.shape[0]) for x in xs]
    dev = xs[0].device
    state = torch.get_rng_state()
    perms = []
    for n in sizes:
        if n == 0:
            raise RuntimeError("spherical_kmeans: x has no rows (the reference's argmax of an empty tensor raises)")
        perms.extend(torch.randperm(n) for _ in range(niter + 1))
    perms = torch.cat(perms).to(torch.int32).to(dev)
    xcat = torch.cat(xs).contiguous() if len(xs) > 1 else xs[0].contiguous()
    offsets = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0).to(dev)
    centers = torch.empty(len(xs), ncluster, D, dtype=torch.float32, device=dev)
    status = torch.empty(len(xs), dtype=torch.int32, device=dev)
    lib = _lib.load()
    rows = sum(sizes)
    ws = torch.empty(max(int(lib.goi_codebook_kmeans_workspace_bytes(rows, len(xs), ncluster, D)), 1), dtype=torch.uint8, device=dev)
    p = ptr
    with torch.cuda.device(dev):
        check(lib.goi_codebook_kmeans(p(xcat), p(offsets), len(xs), max(sizes), rows, D, ncluster, niter, p(perms), p(centers),
                                      p(status), p(ws), stream(dev)), ValueError)
    start = 0
    for x, n in zip(xs, sizes):  # x /= x.norm(...) is in place in the reference
        if xcat.data_ptr() != x.data_ptr():
            x.copy_(xcat[start:start + n])
        start += n
    st = status.cpu().tolist()  # the one synchronisation
    bad = next((i for i, s in enumerate(st) if s), None)
    if bad is not None:
        # the reference raises inside problem `bad` at iteration st[bad] - 1, after its seed draw and st[bad] more
        torch.set_rng_state(state)
        for n in sizes[:bad]:
            for _ in range(niter + 1):
                torch.randperm(n)
        for _ in range(st[bad] + 1):
            torch.randperm(sizes[bad])
        raise RuntimeError(f"spherical_kmeans: more dead centres than the {sizes[bad]} rows at iteration {st[bad] - 1} "
                           f"(the reference's centers[nanix] = x[randperm(N)[:ndead]] shape mismatch)")
    return list(centers.unbind(0))


def spherical_kmeans(x: torch.Tensor, ncluster: int, niter: int = 10) -> torch.Tensor:
    """Device drop-in for io.kmeans (train.py:36-56) on a [N, D] float32 CUDA tensor: spherical_kmeans_batched of one."""
    return spherical_kmeans_batched([x], ncluster, niter)[0]


@torch.no_grad()
def init_codebook(ape_maps, tab_len: int = 300, per_view: int = 80, niter: int = 10) -> torch.Tensor:
    """The code-book initialisation of train.py:78-84 for the [ape_dim, H, W] APE maps given (the caller applies the
    reference's [::8] to its cameras): unique rows per view, k-means of each into per_view centres (one batched launch
    set), k-means of all of them into tab_len; returns the [tab_len, ape_dim] float32 LUT.  Same RNG draws and order as
    the reference stage."""
    uniq = unique_rows(ape_maps)
    tot = torch.cat(spherical_kmeans_batched(uniq, per_view, niter), 0)
    return spherical_kmeans(tot, tab_len, niter).float()
