"""Instance features from per-view 2D masks: the fused mask-contrast loss (csrc/grouping.hip over the C ABI).

    loss(feat, labels, K, margin=1.0, w_intra=1.0, w_inter=1.0, balance="pixel", max_abs=None)  -> 0-d float32, differentiable in `feat`
    loss_terms(...)   -> (loss, intra, inter, grad or None, count int64 [K], qsum int64 [K,S], qexp int32, status int32)
    FeatureView(pc, features)                                                    -> `pc` with `features` as its get_semantics
    fit(cameras, pc, label_maps, K, S=16, iterations=200, lr=0.05, seed=0, normalize=True, eps=1e-8, init_std=0.01, **loss_kw) -> features [P,S]
    instances(xyz, features, seen, tau, k=8, **segment_kw)                        -> segment.Segments

`_semantics` is a language-aligned feature: two chairs side by side carry the same one, `segment.edges` can put no edge between
them at any tau, and `segment.instances` returns one object.  Per-view instance masks (a mask generator's output; their ids mean
nothing across views) say which pixels of ONE view belong together.  The loss trains a second per-Gaussian feature, rendered
through the rasterizer's semantic channel, to be constant inside a mask and at least `margin` apart between the masks of the same
view -- the intra / inter objective of the Gaussian-grouping family:

    feat [S,H,W] float32 as the rasterizer writes `semantics`, labels [H,W] int32; pixel p is in mask m = labels[p] iff 0 <= m < K
    (-1, >= K, INT32_MIN: ignored); n_m pixels in mask m, N = sum n_m, M masks with n_m > 0, mu_m the mean feature of mask m

    L_intra = sum_m a_m sum_{p in m} |f_p - mu_m|^2        a_m = 1/N (balance="pixel")   1/(M n_m) (balance="mask")
    L_inter = 1/(M(M-1)) sum_{m != m', both non-empty} max(0, margin - |mu_m - mu_m'|)^2
    L       = w_intra L_intra + w_inter L_inter

M == 0: L = 0 and a zero gradient; M == 1: L_inter = 0; a pair whose means are equal adds margin^2 and no gradient.  The per-mask
sums are exact integers in units of 2^-qexp (qexp = 40 - e, max|f| < 2^e over the whole map), so they do not depend on any
order; everything after them is float64 in a fixed order: two calls give the same bits.  max_abs: a bound the caller knows on
|feat| (saves the pass that finds the maximum); a pixel at or above the power of two over it saturates and raises bit 0 of
`status`.

float32 tensors on a ROCm GPU only; there is no CPU fallback.  Nothing here synchronises the host.
"""
from __future__ import annotations

import math

import torch

from . import _lib, segment, smooth
from ._lib import check, ptr, stream

_NO_CPU = "goi_hyperplane_amd.grouping: tensors must live on a ROCm GPU; there is no CPU fallback"
S_MAX = 32            # goi_mask_contrast: 1 <= S <= 32
MAX_PIXELS = 2 ** 22  # H * W at most this: the int64 sums cannot overflow
K_MAX = 2 ** 16
BALANCE = {"pixel": 0, "mask": 1}


def _tensor(t, who, what, dtypes):
    if not torch.is_tensor(t):
        raise TypeError(f"grouping.{who}: {what} must be a tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"grouping.{who}: {what} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")
    return t


def _on_gpu(who, **tensors):
    """every given tensor on ONE ROCm GPU"""
    given = {name: t for name, t in tensors.items() if t is not None}
    if any(not t.is_cuda for t in given.values()):
        raise RuntimeError(_NO_CPU)
    first = next(iter(given.values())).device
    for name, t in given.items():
        if t.device != first:
            raise ValueError(f"grouping.{who}: {name} is on {t.device}, expected {first}")


def _finite(v, who, what, lo=None):
    v = float(v)
    if math.isnan(v) or math.isinf(v) or (lo is not None and v < lo):
        raise ValueError(f"grouping.{who}: need a finite {what}" + (f" >= {lo:g}" if lo is not None else ""))
    return v


def _args(feat, labels, K, margin, w_intra, w_inter, balance, max_abs, who="loss"):
    """the checked arguments; where the tensors live is looked at last, so that a wrong dtype or shape is named as such"""
    feat = _tensor(feat, who, "feat", (torch.float32,))
    if feat.dim() != 3 or not 1 <= feat.shape[0] <= S_MAX or feat.shape[1] < 1 or feat.shape[2] < 1:
        raise ValueError(f"grouping.{who}: feat must have shape (S, H, W) with 1 <= S <= {S_MAX} and H, W >= 1")
    labels = _tensor(labels, who, "labels", (torch.int32,))
    if tuple(labels.shape) != tuple(feat.shape[1:]):
        raise ValueError(f"grouping.{who}: labels must have shape {tuple(feat.shape[1:])}, one per pixel of feat")
    if feat.shape[1] * feat.shape[2] > MAX_PIXELS:
        raise ValueError(f"grouping.{who}: need H * W <= 2^22")
    if isinstance(K, bool) or not isinstance(K, int):
        raise TypeError(f"grouping.{who}: K must be an int")
    if not 0 <= K <= K_MAX:
        raise ValueError(f"grouping.{who}: need 0 <= K <= {K_MAX}")
    if balance not in BALANCE:
        raise ValueError(f"grouping.{who}: balance must be 'pixel' or 'mask'")
    margin = _finite(margin, who, "margin", 0.0)
    w_intra, w_inter = _finite(w_intra, who, "w_intra"), _finite(w_inter, who, "w_inter")
    max_abs = -1.0 if max_abs is None else _finite(max_abs, who, "max_abs", 0.0)
    _on_gpu(who, feat=feat, labels=labels)
    return feat, labels.contiguous(), K, margin, w_intra, w_inter, BALANCE[balance], max_abs


def _forward(f, labels, K, margin, w_intra, w_inter, balance, max_abs, want_grad):
    """-> (loss, intra, inter, grad or None, count, qsum, qexp, status), all on the device"""
    lib = _lib.load()
    dev = f.device
    S, H, W = (int(v) for v in f.shape)
    with torch.cuda.device(dev):
        scalars = torch.empty((3,), dtype=torch.float32, device=dev)
        words = torch.empty((2,), dtype=torch.int32, device=dev)
        sums = torch.empty((K, S + 1), dtype=torch.int64, device=dev)  # count | qsum, one allocation
        count, qsum = sums.view(-1)[:K], sums.view(-1)[K:].view(K, S)
        grad = torch.empty((S, H, W), dtype=torch.float32, device=dev) if want_grad else None
        ws = _lib.workspace(lib.goi_mask_contrast_workspace_bytes(S, H, W, K), dev)
        check(lib.goi_mask_contrast(S, H, W, K, ptr(f), ptr(labels), margin, w_intra, w_inter, balance, max_abs, ptr(scalars[0:1]),
                                    ptr(scalars[1:2]), ptr(scalars[2:3]), ptr(grad), ptr(count), ptr(qsum), ptr(words[0:1]),
                                    ptr(words[1:2]), ptr(ws), stream(dev)))
    return scalars[0], scalars[1], scalars[2], grad, count, qsum, words[0], words[1]


class _MaskContrast(torch.autograd.Function):
    """The gradient is formed by the forward (the sums serve both) and saved; the backward is one multiply by the upstream scalar
    on the device."""

    @staticmethod
    def forward(ctx, feat, labels, K, margin, w_intra, w_inter, balance, max_abs):
        out = _forward(feat.detach().contiguous(), labels, K, margin, w_intra, w_inter, balance, max_abs, True)
        ctx.save_for_backward(out[3])
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, g_loss, *_rest):
        (grad,) = ctx.saved_tensors
        return (grad * g_loss,) + (None,) * 7


def loss_terms(feat, labels, K, margin=1.0, w_intra=1.0, w_inter=1.0, balance="pixel", max_abs=None):
    """-> (loss, intra, inter, grad, count, qsum, qexp, status), all on the device: loss = w_intra * intra + w_inter * inter as 0-d
    float32 (`loss` differentiable in `feat`); grad float32 [S,H,W] = dL/dfeat, formed only when feat.requires_grad (else None);
    count int64 [K] and qsum int64 [K,S] the exact per-mask sums in units of 2^-qexp; qexp, status 0-d int32.  See loss()."""
    args = _args(feat, labels, K, margin, w_intra, w_inter, balance, max_abs)
    f = args[0]
    if not (f.requires_grad and torch.is_grad_enabled()):
        return _forward(f.detach().contiguous(), *args[1:], False)
    return _MaskContrast.apply(*args)


def loss(feat, labels, K, margin=1.0, w_intra=1.0, w_inter=1.0, balance="pixel", max_abs=None):
    """-> 0-d float32: L = w_intra L_intra + w_inter L_inter (module docstring) of one view, with its gradient to `feat` only.

        out = render.render(cam, grouping.FeatureView(pc, features), pipe, black)
        grouping.loss(out["semantics"], label_map, K).backward()

    feat: float32 [S,H,W], 1 <= S <= 32, H * W <= 2^22; labels: int32 [H,W]; K: an upper bound on the view's mask ids (ids outside
    [0, K) are ignored).  The forward computes and saves the gradient when feat.requires_grad and computes none otherwise; the
    backward is one multiply.  Two calls give the same bits.  No host synchronisation in forward or backward."""
    return loss_terms(feat, labels, K, margin, w_intra, w_inter, balance, max_abs)[0]


class FeatureView:
    """`pc` with `features` [P,S] as its get_semantics: render.render(camera, FeatureView(pc, features), ...) draws the instance
    feature through the semantic channel, and everything else is pc's.  frozen=True hands out pc's tensors detached (made once,
    so that they keep their identity from frame to frame): only `features` can then receive a gradient and the backward skips
    the geometry."""

    _TENSORS = ("get_xyz", "get_scaling", "get_rotation", "get_opacity", "get_features")

    def __init__(self, pc, features, frozen=False):
        if not torch.is_tensor(features) or features.dim() != 2 or features.shape[0] != pc.get_xyz.shape[0]:
            raise ValueError("grouping.FeatureView: features must have shape (P, S), one row per Gaussian of pc")
        self._pc, self._features = pc, features
        self._held = {name: getattr(pc, name).detach() for name in self._TENSORS} if frozen else {}

    @property
    def get_semantics(self):
        return self._features

    def __getattr__(self, name):  # (only what the instance itself does not have)
        held = self.__dict__.get("_held", {})
        return held[name] if name in held else getattr(self.__dict__["_pc"], name)


def fit(cameras, pc, label_maps, K, S=16, iterations=200, lr=0.05, seed=0, pipe=None, normalize=True, eps=1e-8, init_std=0.01,
        **loss_kw):
    """-> features float32 [P,S]: an instance feature per Gaussian, trained so that every view's rendered feature map is constant
    inside each of the view's masks and `margin` apart between them.  label_maps: one int32 [H,W] per camera (its ids need not
    agree with any other view's).  Iteration i renders camera i mod len(cameras) through FeatureView(pc, features, frozen=True) on a
    black background, applies loss(..., **loss_kw) and steps optim.FusedAdam(lr, eps) on `features` alone; nothing is read back
    inside the loop.
    normalize=True divides the rendered map by the frame's alpha (clamped at 1e-3) first: the rasterizer writes sum_i w_i f_i
    with sum_i w_i = alpha, so without it a mask's thin rim could only reach the mask's mean by growing the rim Gaussians'
    features like 1 / alpha, which tears the mask's Gaussians apart instead of gathering them.
    eps is Adam's: at 1e-8 a Gaussian that hardly any pixel blends is moved by lr per step along a gradient that hardly changes
    the picture and drifts away from its neighbours; a larger eps (1e-4) leaves it near where it started.
    The features start as N(0, init_std^2) from torch.Generator(seed) on the CPU (the same on every device): all-zero features
    are a fixed point of the loss -- every mean coincides, such a pair has no gradient, and the intra term is already 0 -- so a
    zero initialisation never moves.  The component of the initial noise that averages out in every pixel is never trained
    away, which is why it is small.  A Gaussian no labelled pixel blends keeps its initial row: see instances()."""
    from . import optim, render
    cameras, label_maps = list(cameras), list(label_maps)
    if not cameras or len(cameras) != len(label_maps):
        raise ValueError("grouping.fit: need one label map per camera, and at least one camera")
    if isinstance(S, bool) or not isinstance(S, int) or not 1 <= S <= S_MAX:
        raise ValueError(f"grouping.fit: need 1 <= S <= {S_MAX}")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 0:
        raise ValueError("grouping.fit: iterations must be an int >= 0")
    xyz = pc.get_xyz
    if not xyz.is_cuda:
        raise RuntimeError(_NO_CPU)
    dev = xyz.device
    maps = [_tensor(m, "fit", "a label map", (torch.int32,)).contiguous() for m in label_maps]
    _on_gpu("fit", xyz=xyz, **{f"label_maps[{i}]": m for i, m in enumerate(maps)})
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    init = torch.randn((int(xyz.shape[0]), S), generator=gen, dtype=torch.float32) * float(init_std)
    features = torch.nn.Parameter(init.to(dev))
    view = FeatureView(pc, features, frozen=True)
    opt = optim.FusedAdam([features], lr=lr, eps=eps)
    pipe = render.PipelineParams() if pipe is None else pipe
    black = torch.zeros(3, dtype=torch.float32, device=dev)
    for it in range(iterations):
        i = it % len(cameras)
        opt.zero_grad(set_to_none=True)
        out = render.render(cameras[i], view, pipe, black)
        sem = out["semantics"]
        if normalize:
            sem = sem / out["alpha"].detach().reshape(1, *sem.shape[1:]).clamp_min(1e-3)
        loss(sem, maps[i], K, **loss_kw).backward()
        opt.step()
    return features.detach()


def instances(xyz, features, seen, tau, k=8, **segment_kw):
    """-> segment.Segments: smooth.complete_features(xyz, features, seen, k) fills the rows with seen == 0 (the Gaussians no
    labelled pixel trained) from their neighbours, then segment.instances(xyz, completed, k=k, tau=tau, **segment_kw).  tau is
    segment.edges' largest SQUARED feature distance inside an object."""
    completed = smooth.complete_features(xyz, features, seen, k=k)
    return segment.instances(xyz, completed, k=k, tau=tau, **segment_kw)
