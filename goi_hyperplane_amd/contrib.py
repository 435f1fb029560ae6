"""What a capture actually uses, what is under a pixel, and which Gaussians a 2D label map means, read off the blend itself
(csrc/contrib.hip).

    frame(camera, pc, bg_color, ...)           -> ContribFrame(peak [P], top_id [H,W], top_w [H,W]) of one view
    peak_weights(cameras, pc, bg_color, ...)   -> float32 [P]: the largest blend weight alpha * T of every Gaussian over a camera set
    pick(camera, pc, bg_color, xy, ...)        -> int64: the dominant Gaussian under the given pixel(s), -1 for none
    prune_unseen(g, cameras, bg_color, min_weight=0.0, ...) -> bool [P]: prunes what the camera set never (or hardly) shows
    frame_votes(camera, pc, bg_color, labels, K, ...) / votes(cameras, pc, bg_color, labels, K, ...)
                                               -> int64 [P, K]: the sum of alpha * T of every Gaussian over the pixels of each label
    assign(votes, min_weight=0.0)              -> (label int64 [P], share float32 [P]): the class with the most votes
    lift_mask(cameras, pc, bg_color, masks, threshold=0.5, min_weight=0.0, ...) -> bool [P]: the Gaussians a set of 2D masks means

VOTES lift 2D label maps (a segmentation mask, relevant_cameras' masks, ground truth) onto the Gaussians by how much each adds
to the labelled pixels: for every pair that CONTRIBUTES to a pixel whose label l is in [0, K) (anything else is ignored),
votes[g, l] += round(alpha * T * 2^24), half-to-even.  The stopper is excluded here (it added nothing to the picture), which
makes the sums those of a backward with a one-hot upstream on K channels -- without the trainable forward, the row scratch, the
limit of S labels per pass or fp32 sums.  Integer sums by 64-bit atomics: order-free, the same bits every run and in any camera
order.  VOTE_ONE = 2^24 is one pixel's full weight; every contribution is at least 1 unit, so a Gaussian's total is non-zero
exactly when it contributed to a validly labelled pixel.

The peak weight is RadSplat's importance score.  It is not obtainable from the differentiable path (a backward with a constant
upstream gives SUMS of weights) and neither mark_visible nor radii > 0 says more than "in the frustum".  The rule, per pixel:
the tile's depth-ordered list is walked as the forward walks it; a pair that passes both alpha guards on a pixel that is still
live has w = alpha * T.  `peak` takes the maximum of w over contributors and over the pair that ENDED the pixel (the stopper:
its w is what the Gaussian would have added), `top_id` / `top_w` the contributor of largest w (the front-most of equals; the
stopper added nothing to the picture and is excluded).  Because the stopper counts, a Gaussian whose peak is 0 over a camera
set never passed the guards on a live pixel of any of those frames: removing it changes no pixel's sequence of live hits, hence
no output map, in any bit -- prune_unseen(min_weight=0) is free.

Every view costs one exact forward, whose count of listed instances is read back by the host: the one synchronisation per
view (as in the reference's forward).  A read-back-free sweep through the speculative forward is not provided.  The merge into
`peak` is an integer atomic maximum on the bit patterns of non-negative floats: order-free, the same bits every run.  fp32
tensors on a ROCm GPU only; there is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import _C, _lib
from ._lib import check, ptr, stream

_NO_CPU = "goi_hyperplane_amd.contrib: tensors must live on a ROCm GPU; there is no CPU fallback"


class ContribFrame(NamedTuple):
    peak: torch.Tensor    # [P] float32, max-merged
    top_id: torch.Tensor  # [H,W] int32 (None with want_ids=False)
    top_w: torch.Tensor   # [H,W] float32 (None with want_ids=False)


def frame_buffers(P, W, H, R, geom, binning, img, peak=None, want_ids=True) -> ContribFrame:
    """goi_raster_contrib_frame on the workspaces a forward returned (R: its num_rendered, an int or the LazyCount of a
    speculative frame, which is resolved here).  peak: float32 [P] on the device to merge into (None: a fresh zeroed one)."""
    lib = _lib.load()
    if not geom.is_cuda:
        raise RuntimeError(_NO_CPU)
    dev = geom.device
    int(R)  # (resolves -- and, after an overflow, redoes -- a speculative frame)
    R, lazy_binning = _C._layout_of(R)
    if lazy_binning is not None:
        binning = lazy_binning
    if peak is None:
        peak = torch.zeros(P, dtype=torch.float32, device=dev)
    elif not torch.is_tensor(peak) or peak.dtype != torch.float32 or tuple(peak.shape) != (P,) or not peak.is_contiguous():
        raise ValueError(f"contrib: peak must be a contiguous float32 tensor of shape ({P},)")
    elif not peak.is_cuda:
        raise RuntimeError(_NO_CPU)
    elif peak.device != dev:
        raise ValueError(f"contrib: peak is on {peak.device}, expected {dev}")
    top_id = top_w = None
    with torch.cuda.device(dev):
        if want_ids:
            top_id = torch.empty((H, W), dtype=torch.int32, device=dev)
            top_w = torch.empty((H, W), dtype=torch.float32, device=dev)
        check(lib.goi_raster_contrib_frame(P, W, H, R, ptr(geom), ptr(binning), ptr(img), ptr(peak), ptr(top_id), ptr(top_w),
                                           stream(dev)))
    return ContribFrame(peak, top_id, top_w)


def _exact_forward(camera, pc, bg_color, scaling_modifier, gaussian_mask, who):
    """The exact forward of `pc` from `camera` that frame() and frame_votes() replay -> (P, W, H, n, geom, binning, img)"""
    xyz = pc.get_xyz
    if not xyz.is_cuda or not bg_color.is_cuda:
        raise RuntimeError(_NO_CPU)
    P, H, W = int(xyz.shape[0]), int(camera.image_height), int(camera.image_width)
    if P == 0:
        raise ValueError(f"contrib.{who}: the model has no Gaussians")
    d = lambda t: t.detach()  # noqa: E731
    args = (bg_color, d(xyz), torch.Tensor([]), d(pc.get_semantics), d(pc.get_opacity), d(pc.get_scaling), d(pc.get_rotation),
            float(scaling_modifier), torch.Tensor([]), camera.world_view_transform, camera.full_proj_transform,
            math.tan(camera.FoVx * 0.5), math.tan(camera.FoVy * 0.5), H, W, d(pc.get_features), int(pc.active_sh_degree),
            camera.camera_center, False, False)
    was = getattr(_C._CALL, "inference", False)
    _C._CALL.inference = True  # an image-only frame: the exact forward
    try:
        if gaussian_mask is None:
            n, *_maps, geom, binning, img = _C.rasterize_gaussians(*args)
        else:
            n, *_maps, geom, binning, img = _C.rasterize_gaussians_selected(*args, gaussian_mask, False)
    finally:
        _C._CALL.inference = was
    return P, W, H, n, geom, binning, img


def frame(camera, pc, bg_color, *, scaling_modifier=1.0, gaussian_mask=None, peak=None, want_ids=True) -> ContribFrame:
    """One view: an exact forward of `pc` from `camera` (render()'s operands: SH colours, scale + rotation), then the replay of
    that frame.  peak: the array to merge into (float32 [P]; None: zeros).  gaussian_mask (bool / uint8 [P], contiguous): the
    frame is the in-place selected forward's, and an unselected Gaussian keeps its `peak` untouched.  want_ids=False skips the
    two per-pixel maps.  Costs the exact forward's one read-back of its instance count; nothing else synchronises."""
    return frame_buffers(*_exact_forward(camera, pc, bg_color, scaling_modifier, gaussian_mask, "frame"), peak, want_ids)


def peak_weights(cameras, pc, bg_color, **kw) -> torch.Tensor:
    """float32 [P]: the largest blend weight of every Gaussian over every pixel of every camera (sizes may differ): one zeroed
    array, one frame() per camera in order.  Bit-identical for any camera order.  One read-back (the forward's count) per view."""
    if not pc.get_xyz.is_cuda:
        raise RuntimeError(_NO_CPU)
    kw.pop("want_ids", None)
    peak = kw.pop("peak", None)
    if peak is None:
        peak = torch.zeros(int(pc.get_xyz.shape[0]), dtype=torch.float32, device=pc.get_xyz.device)
    for cam in cameras:
        frame(cam, pc, bg_color, peak=peak, want_ids=False, **kw)
    return peak


def pick(camera, pc, bg_color, xy, **kw) -> torch.Tensor:
    """The dominant contributor under pixel(s) xy = (x, y) or [n,2] (ints, or an integer tensor on the device): an int64 device
    tensor ([] or [n]), -1 where nothing contributed.  Adds no synchronisation to frame()'s one read-back."""
    f = frame(camera, pc, bg_color, **kw)
    dev = f.top_id.device
    if torch.is_tensor(xy):
        if not xy.is_cuda:
            raise RuntimeError(_NO_CPU)
        xy = xy.to(torch.int64)
    else:
        xy = torch.tensor(xy, dtype=torch.int64).to(dev, non_blocking=True)
    if xy.shape[-1:] != (2,) or xy.dim() > 2:
        raise ValueError("contrib.pick: xy must be (x, y) or [n,2]")
    return f.top_id[xy[..., 1], xy[..., 0]].to(torch.int64)


def prune_unseen(g, cameras, bg_color, min_weight=0.0, **kw) -> torch.Tensor:
    """Prunes the Gaussians a camera set does not use and returns the prune mask (bool [P], True = removed): peak <= 0 for
    min_weight == 0 -- provably free: every output map of every one of `cameras` keeps its bits -- else peak < min_weight.
    Applied with densify.prune_points(g, mask): Adam moments, statistics and row order follow its contract.  `g`: a model with
    the reference GaussianModel's attributes and accessors.  One read-back per view plus prune_points' one."""
    from . import densify
    if min_weight < 0:
        raise ValueError("contrib.prune_unseen: min_weight must be >= 0")
    peak = peak_weights(cameras, g, bg_color, **kw)
    mask = (peak <= 0.0) if min_weight == 0 else (peak < float(min_weight))
    densify.prune_points(g, mask)
    return mask


VOTE_ONE = 1 << 24  # votes are integers in units of 2^-24 of one pixel's full blend weight


def votes_buffers(P, W, H, R, geom, binning, img, labels, K, votes=None) -> torch.Tensor:
    """goi_raster_contrib_votes on the workspaces a forward returned (R as for frame_buffers).  labels: an integer or bool
    tensor of H*W elements on the device (converted to contiguous int32; values outside [0, K) are ignored).  votes: int64
    [P, K] on the device to ADD to (None: a fresh zeroed one).  -> votes."""
    lib = _lib.load()
    if not geom.is_cuda:
        raise RuntimeError(_NO_CPU)
    dev = geom.device
    K = int(K)
    int(R)  # (resolves -- and, after an overflow, redoes -- a speculative frame)
    R, lazy_binning = _C._layout_of(R)
    if lazy_binning is not None:
        binning = lazy_binning
    if not torch.is_tensor(labels) or labels.is_floating_point() or labels.is_complex() or labels.numel() != H * W:
        raise ValueError(f"contrib: labels must be an integer or bool tensor of {H} x {W} elements")
    if not labels.is_cuda:
        raise RuntimeError(_NO_CPU)
    if labels.device != dev:
        raise ValueError(f"contrib: labels is on {labels.device}, expected {dev}")
    if K < 1:
        raise ValueError("contrib: K must be at least 1")
    labels = labels.to(torch.int32).contiguous()
    if votes is None:
        votes = torch.zeros((P, K), dtype=torch.int64, device=dev)
    elif not torch.is_tensor(votes) or votes.dtype != torch.int64 or tuple(votes.shape) != (P, K) or not votes.is_contiguous():
        raise ValueError(f"contrib: votes must be a contiguous int64 tensor of shape ({P}, {K})")
    elif not votes.is_cuda:
        raise RuntimeError(_NO_CPU)
    elif votes.device != dev:
        raise ValueError(f"contrib: votes is on {votes.device}, expected {dev}")
    with torch.cuda.device(dev):
        check(lib.goi_raster_contrib_votes(P, W, H, R, ptr(geom), ptr(binning), ptr(img), ptr(labels), K, ptr(votes), stream(dev)))
    return votes


def frame_votes(camera, pc, bg_color, labels, K, *, scaling_modifier=1.0, gaussian_mask=None, votes=None) -> torch.Tensor:
    """One view: the exact forward frame() runs, then the votes of that frame for the view's label map (votes_buffers).  With
    gaussian_mask an unselected Gaussian keeps its row of `votes` untouched.  One read-back (the forward's count)."""
    return votes_buffers(*_exact_forward(camera, pc, bg_color, scaling_modifier, gaussian_mask, "frame_votes"), labels, K, votes)


def _per_camera(maps, n, what):
    """The label map (or mask) of each of n cameras, from a sequence or a [V,H,W] / [V,1,H,W] tensor"""
    if torch.is_tensor(maps):
        if maps.dim() == 4 and maps.shape[1] == 1:
            maps = maps[:, 0]
        if maps.dim() != 3:
            raise ValueError(f"contrib: {what} must be a sequence of per-camera maps or a [V,H,W] / [V,1,H,W] tensor")
    if len(maps) != n:
        raise ValueError(f"contrib: {len(maps)} {what} for {n} cameras")
    return maps


def votes(cameras, pc, bg_color, labels, K, **kw) -> torch.Tensor:
    """int64 [P, K]: every Gaussian's blend weight on the pixels of each label, summed over every camera, in units of
    2^-24 (VOTE_ONE = one pixel's full weight).  labels: one map per camera (a sequence -- camera sizes may differ -- or a
    [V,H,W] / [V,1,H,W] tensor).  One array swept over the cameras in order; integer sums: bit-identical for any camera
    order.  One read-back (the forward's count) per view."""
    if not pc.get_xyz.is_cuda:
        raise RuntimeError(_NO_CPU)
    cameras = list(cameras)
    labels = _per_camera(labels, len(cameras), "label maps")
    out = kw.pop("votes", None)
    if out is None:
        out = torch.zeros((int(pc.get_xyz.shape[0]), int(K)), dtype=torch.int64, device=pc.get_xyz.device)
    for cam, lab in zip(cameras, labels):
        frame_votes(cam, pc, bg_color, lab, K, votes=out, **kw)
    return out


def _assign(votes, min_weight):
    total = votes.sum(dim=1)
    best = votes.max(dim=1).values
    # the LOWEST class among those with the most votes, stated here and not left to a library's tie rule
    classes = torch.arange(votes.shape[1], dtype=torch.int64, device=votes.device)
    label = torch.where(votes == best[:, None], classes[None, :], votes.shape[1]).min(dim=1).values
    none = (total <= 0) | (total.double() < float(min_weight) * VOTE_ONE)
    share = torch.where(none, 0.0, best.double() / total.clamp(min=1).double()).float()
    return torch.where(none, -1, label), share


def assign(votes, min_weight=0.0):
    """-> (label int64 [P], share float32 [P]) of a votes array: the class with the most votes, the LOWEST class among equals;
    -1 where the Gaussian has no vote or fewer than min_weight pixels' worth (total < min_weight * VOTE_ONE).  share = best /
    total (computed in float64), 0 where label is -1."""
    if not torch.is_tensor(votes) or votes.dtype != torch.int64 or votes.dim() != 2 or votes.shape[1] < 1:
        raise ValueError("contrib.assign: votes must be an int64 tensor of shape (P, K)")
    if not votes.is_cuda:
        raise RuntimeError(_NO_CPU)
    return _assign(votes, min_weight)


def _lift(votes, threshold, min_weight):
    inside, total = votes[:, 1].double(), votes.sum(dim=1).double()
    return (total > 0) & (total >= float(min_weight) * VOTE_ONE) & (inside > float(threshold) * total)


def lift_mask(cameras, pc, bg_color, masks, threshold=0.5, min_weight=0.0, **kw) -> torch.Tensor:
    """bool [P]: the Gaussians a set of 2D masks means.  masks: one per camera (a sequence, or a [V,H,W] / [V,1,H,W] tensor such
    as RelevantCameras.semantic_mask); a pixel is IN where mask != 0.  Votes with K = 2; a Gaussian is selected iff it has a
    vote, total >= min_weight * VOTE_ONE and in > threshold * total (float64 on the device)."""
    if not pc.get_xyz.is_cuda:
        raise RuntimeError(_NO_CPU)
    cameras = list(cameras)
    masks = _per_camera(masks, len(cameras), "masks")
    for m in masks:
        if not torch.is_tensor(m) or not m.is_cuda:
            raise RuntimeError(_NO_CPU)
    return _lift(votes(cameras, pc, bg_color, [(m != 0) for m in masks], 2, **kw), threshold, min_weight)
