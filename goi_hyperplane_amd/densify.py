"""Densification and pruning of the Gaussian set on the device (csrc/densify.hip): the methods of the reference's
GaussianModel that change the number of Gaussians P (scene/gaussian_model.py:291-513).

    add_densification_stats(g, viewspace_point_tensor, update_filter)                     :512-514
    densify_and_prune(g, max_grad, min_opacity, extent, max_screen_size, generator=None)  :496-510 (with :432-494)
    prune_points(g, mask)                                                                 :393-408 (GOI's 3D delete)
    reset_opacity(g)                                                                      :291-294 (with :360-373)

`g` is any object with the reference GaussianModel's attributes -- the reference's own instance works unchanged:
parameters _xyz [P,3], _features_dc [P,1,3], _features_rest [P,M-1,3], _semantics [P,S], _opacity [P,1], _scaling [P,3],
_rotation [P,4] (raw: scaling through exp, opacity through sigmoid, rotation through build_rotation); statistics
xyz_gradient_accum [P,1], denom [P,1], max_radii2D [P]; percent_dense, optimizer and _semantics_masks.

densify_and_prune gives the rows, in the order, of the reference's clone -> split -> prune-parents -> prune sequence:
[originals not split, not pruned] [clones not pruned] [first children not pruned] [second children not pruned].  Copied
rows are bit-exact; the children's positions go through torch.bmm in the reference and a fixed FMA chain here (a few ulp).
The normal draws Z come from `generator` (or the device's default generator) exactly as torch.normal consumes it.  The
optimizer (torch.optim.Adam or FusedAdam, groups named xyz / f_dc / f_rest / semantics / opacity / scaling / rotation) is
re-keyed as _prune_optimizer / cat_tensors_to_optimizer do it: kept rows keep exp_avg / exp_avg_sq, new rows get zeros,
`step` is untouched, group["params"][0] becomes a new nn.Parameter.

Deliberate differences from the reference, all where it raises (or would go on with a broken model):
  * a parameter without an optimizer group, or optimizer None, is still compacted / extended (the reference raises
    KeyError / AttributeError -- what GOI's GUI meets: finetune_sh_setup builds a partial group list, and edit_delete can
    run before any training);
  * prune_points leaves a statistic that was never set up as it is (a model from the reference's load_ply keeps
    xyz_gradient_accum / denom at torch.empty(0); the reference's prune_points raises IndexError there);
  * reset_opacity without an optimizer, without an "opacity" group or without optimizer state for it just sets the new
    opacities (the reference raises AttributeError, KeyError or TypeError);
  * a model whose _semantics_masks is set is refused with ValueError (the reference would keep the mask at the old P).

densify_and_prune and prune_points read the new row counts back once (the new tensors' shapes live on the host): their
only host synchronisation.  add_densification_stats and reset_opacity do not synchronise.  fp32 tensors on a ROCm GPU
only; there is no CPU fallback.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib
from ._lib import check, ptr, stream, workspace

_NO_CPU = "goi_hyperplane_amd.densify: tensors must live on a ROCm GPU; there is no CPU fallback"

# optimizer group name -> model attribute (scene/gaussian_model.py:168-176)
PARAMS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("semantics", "_semantics"),
          ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))
_ATTR = dict(PARAMS)
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
_PARAM, _MOMENT, _XYZ, _SCALING, _ZERO = 0, 1, 2, 3, 4  # GOI_DENSIFY_* of include/goi_raster.h
_ROW = {"_xyz": (3,), "_opacity": (1,), "_scaling": (3,), "_rotation": (4,)}  # the row shapes the kernels read


def _check(t, what, fn, dev=None):
    if not torch.is_tensor(t):
        raise TypeError(f"{fn}: {what} must be a tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{fn}: {what} must be torch.float32, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(_NO_CPU)
    if dev is not None and t.device != dev:
        raise ValueError(f"{fn}: {what} is on {t.device}, expected {dev}")
    if not t.is_contiguous():
        raise ValueError(f"{fn}: {what} must be contiguous")


def _params(g, fn):
    """The 7 parameters {attr: tensor}, checked; P; device."""
    if getattr(g, "_semantics_masks", None) is not None:
        raise ValueError(f"{fn}: the model has a semantic mask set (set_semantic_masks); it would keep the old number of "
                         "Gaussians -- clear it (set_semantic_masks(None)) first")
    _check(g._xyz, "_xyz", fn)
    dev = g._xyz.device
    P = int(g._xyz.shape[0]) if g._xyz.dim() else -1
    out = {}
    for _, attr in PARAMS:
        t = getattr(g, attr)
        _check(t, attr, fn, dev)
        if t.dim() < 1 or t.shape[0] != P or (attr in _ROW and tuple(t.shape[1:]) != _ROW[attr]):
            raise ValueError(f"{fn}: {attr} has shape {tuple(t.shape)} (P = {P} from _xyz)")
        out[attr] = t
    return out, P, dev


def _stats(g, P, dev, fn, optional):
    """{name: tensor} of the three statistics; with `optional`, one that was never set up (empty, as a model loaded from
    a .ply has them) maps to None and is left as it is."""
    out = {}
    for name in STATS:
        t = getattr(g, name, None)
        want = (P,) if name == "max_radii2D" else (P, 1)
        if optional and (t is None or (torch.is_tensor(t) and t.numel() == 0 and tuple(t.shape) != want)):
            out[name] = None
            continue
        _check(t, name, fn, dev)
        if tuple(t.shape) != want:
            raise ValueError(f"{fn}: {name} has shape {tuple(t.shape)}, expected {want}")
        out[name] = t
    return out


def _groups(g, fn):
    """(optimizer or None, {group name: group}) with every group checked against the model."""
    opt = getattr(g, "optimizer", None)
    if opt is None:
        return None, {}
    groups = {}
    for group in opt.param_groups:
        name = group.get("name")
        if name not in _ATTR:
            raise ValueError(f"{fn}: optimizer group {name!r} is not one of the model's parameters {tuple(_ATTR)}")
        if name in groups:
            raise ValueError(f"{fn}: two optimizer groups are named {name!r}")
        if len(group["params"]) != 1:
            raise ValueError(f"{fn}: optimizer group {name!r} holds {len(group['params'])} tensors, expected 1")
        if group["params"][0] is not getattr(g, _ATTR[name]):
            raise ValueError(f"{fn}: optimizer group {name!r} does not hold the model's {_ATTR[name]}")
        groups[name] = group
    return opt, groups


def _moments(opt, group, p, fn, name):
    """(the parameter's state dict or None, (exp_avg, exp_avg_sq) or None)"""
    if opt is None or group is None:
        return None, None
    st = opt.state.get(p, None)
    if not st or "exp_avg" not in st:
        return st, None
    mv = (st["exp_avg"], st["exp_avg_sq"])
    for what, t in zip(("exp_avg", "exp_avg_sq"), mv):
        _check(t, f"the {what} of group {name!r}", fn, p.device)
        if t.shape != p.shape:
            raise ValueError(f"{fn}: the {what} of group {name!r} has shape {tuple(t.shape)}, expected {tuple(p.shape)}")
    return st, mv


def _plan_workspace(lib, P, dev, fn):
    nbytes = int(lib.goi_raster_densify_workspace_bytes(P))
    if nbytes == 0:
        raise ValueError(f"{fn}: P = {P} is out of range (P < 2^30)")
    return workspace(nbytes, dev)


def _row_len(t):
    n = 1
    for s in t.shape[1:]:
        n *= int(s)
    return n


def _draw_z(n_split, dev, generator):
    """Z [2 n_split, 3]: torch.normal(mean=zeros, std=stds) is normal_(0, 1) on its output, then mul_(std), add_(mean)"""
    z = torch.empty((2 * n_split, 3), dtype=torch.float32, device=dev)
    return z.normal_(0.0, 1.0, generator=generator)


def _rebuild(g, fn, lib, P, P_new, params, opt, groups, moments, stats, stats_zero, ws, dev, z=None, n_split=0,
             kept_children=0):
    """One apply launch into freshly allocated tensors of P_new rows, then the model and optimizer re-keyed."""
    rows, new, new_mv, new_stats = [], {}, {}, {}
    for name, attr in PARAMS:
        src = params[attr]
        dst = torch.empty((P_new,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
        new[attr] = dst
        rl = _row_len(src)
        mode = _XYZ if attr == "_xyz" else _SCALING if attr == "_scaling" else _PARAM
        if rl:
            rows.append(_lib.GoiDensifyRows(src.data_ptr(), dst.data_ptr(), P, rl, mode))
        mv = moments[name][1]
        if mv is not None:
            new_mv[name] = (torch.empty_like(dst), torch.empty_like(dst))
            if rl:
                rows += [_lib.GoiDensifyRows(s.data_ptr(), d.data_ptr(), P, rl, _MOMENT) for s, d in zip(mv, new_mv[name])]
    for name in STATS:
        t = stats[name]
        if t is None:
            continue
        d = torch.empty((P_new,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        new_stats[name] = d
        rows.append(_lib.GoiDensifyRows(None, d.data_ptr(), P_new, 1, _ZERO) if stats_zero else
                    _lib.GoiDensifyRows(t.data_ptr(), d.data_ptr(), P, 1, _PARAM))
    if P_new > 0 and rows:
        arr = (_lib.GoiDensifyRows * len(rows))(*rows)
        with torch.cuda.device(dev):
            check(lib.goi_raster_densify_apply(P, arr, len(rows), ptr(params["_rotation"]), ptr(params["_scaling"]), ptr(z), n_split,
                                               kept_children, ptr(ws), stream(dev)), ValueError)
    for name, attr in PARAMS:
        old, t, group = params[attr], new[attr], groups.get(name)
        if group is None:
            keep_grad = old.requires_grad
            setattr(g, attr, nn.Parameter(t, requires_grad=keep_grad) if isinstance(old, nn.Parameter) else
                    t.requires_grad_(keep_grad))
            continue
        p = nn.Parameter(t.requires_grad_(True))
        st = moments[name][0]
        if st is not None:
            if name in new_mv:
                st["exp_avg"], st["exp_avg_sq"] = new_mv[name]
            del opt.state[old]
            opt.state[p] = st
        group["params"][0] = p
        setattr(g, attr, p)
    for name, t in new_stats.items():
        setattr(g, name, t)


def densify_and_prune(g, max_grad, min_opacity, extent, max_screen_size, generator=None) -> None:
    """GaussianModel.densify_and_prune: clone, split and prune in one plan + one apply (see the module docstring).
    Afterwards xyz_gradient_accum, denom and max_radii2D are zeros of the new length."""
    fn = "densify_and_prune"
    params, P, dev = _params(g, fn)
    stats = _stats(g, P, dev, fn, optional=False)
    opt, groups = _groups(g, fn)
    moments = {name: _moments(opt, groups.get(name), params[attr], fn, name) for name, attr in PARAMS}
    lib = _lib.load()
    ws = _plan_workspace(lib, P, dev, fn)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    screen = bool(max_screen_size)
    with torch.cuda.device(dev):
        # thresholds formed in Python double arithmetic, as the reference forms them
        check(lib.goi_raster_densify_plan(P, ptr(stats["xyz_gradient_accum"]), ptr(stats["denom"]), ptr(params["_scaling"]),
                                          ptr(params["_opacity"]), float(max_grad), float(g.percent_dense * extent),
                                          float(min_opacity), 1 if screen else 0, float(max_screen_size) if screen else 0.0,
                                          float(0.1 * extent), ptr(counts), ptr(ws), stream(dev)), ValueError)
    kept, clones, children, n_split = (int(c) for c in counts.tolist())  # the one host synchronisation
    z = _draw_z(n_split, dev, generator)
    _rebuild(g, fn, lib, P, kept + clones + 2 * children, params, opt, groups, moments, stats, True, ws, dev, z, n_split,
             children)


def prune_points(g, mask) -> None:
    """GaussianModel.prune_points: removes the Gaussians where `mask` (bool or uint8 [P], on the device) is true from the 7
    parameters, their Adam moments and the three statistics (values kept).  GOI's 3D delete (gui/main.py:515-523,
    edit_delete) is prune_points(g, selection); extracting the selection alone is prune_points(g, ~selection)."""
    fn = "prune_points"
    params, P, dev = _params(g, fn)
    stats = _stats(g, P, dev, fn, optional=True)
    opt, groups = _groups(g, fn)
    moments = {name: _moments(opt, groups.get(name), params[attr], fn, name) for name, attr in PARAMS}
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (P,):
        raise ValueError(f"{fn}: mask must be a bool or uint8 tensor of shape ({P},)")
    if not mask.is_cuda:
        raise RuntimeError(_NO_CPU)
    if mask.device != dev:
        raise ValueError(f"{fn}: mask is on {mask.device}, expected {dev}")
    mask = mask.contiguous()
    lib = _lib.load()
    ws = _plan_workspace(lib, P, dev, fn)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.goi_raster_densify_prune_plan(P, ptr(mask), ptr(counts), ptr(ws), stream(dev)), ValueError)
    kept = int(counts[0].item())  # the one host synchronisation
    _rebuild(g, fn, lib, P, kept, params, opt, groups, moments, stats, False, ws, dev)


def add_densification_stats(g, viewspace_point_tensor, update_filter) -> None:
    """GaussianModel.add_densification_stats: for the rows where update_filter (bool / uint8 [P]) is true,
    xyz_gradient_accum += |viewspace_point_tensor.grad[:, :2]| and denom += 1.  One kernel, no host synchronisation."""
    fn = "add_densification_stats"
    grad = viewspace_point_tensor.grad
    if grad is None:
        raise ValueError(f"{fn}: viewspace_point_tensor.grad is None -- the backward left no 2-D mean gradient (the "
                         "rasterizer's accumulate mode gives autograd none); densification statistics need a per-view backward")
    accum, denom = g.xyz_gradient_accum, g.denom
    _check(accum, "xyz_gradient_accum", fn)
    dev = accum.device
    _check(denom, "denom", fn, dev)
    P = int(accum.shape[0]) if accum.dim() else -1
    if tuple(accum.shape) != (P, 1) or tuple(denom.shape) != (P, 1):
        raise ValueError(f"{fn}: xyz_gradient_accum / denom must be [P, 1], got {tuple(accum.shape)} / {tuple(denom.shape)}")
    if grad.dtype != torch.float32:
        raise TypeError(f"{fn}: the gradient must be torch.float32, got {grad.dtype}")
    if not grad.is_cuda:
        raise RuntimeError(_NO_CPU)
    if grad.device != dev or grad.dim() != 2 or grad.shape[0] != P or grad.shape[1] < 2:
        raise ValueError(f"{fn}: viewspace_point_tensor.grad must be [{P}, >= 2] on {dev}, got {tuple(grad.shape)} on {grad.device}")
    if grad.stride(1) != 1 or grad.stride(0) < 2:
        grad = grad.contiguous()
    if not torch.is_tensor(update_filter) or update_filter.dtype not in (torch.bool, torch.uint8) or \
            tuple(update_filter.shape) != (P,):
        raise ValueError(f"{fn}: update_filter must be a bool or uint8 tensor of shape ({P},)")
    if not update_filter.is_cuda:
        raise RuntimeError(_NO_CPU)
    if update_filter.device != dev:
        raise ValueError(f"{fn}: update_filter is on {update_filter.device}, expected {dev}")
    filt = update_filter.contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.goi_raster_densify_stats(P, ptr(grad), int(grad.stride(0)), ptr(filt), ptr(accum), ptr(denom), stream(dev)),
              ValueError)


@torch.no_grad()
def reset_opacity(g) -> None:
    """GaussianModel.reset_opacity: _opacity = inverse_sigmoid(min(sigmoid(_opacity), 0.01)) with the opacity group's
    moments zeroed and the group re-keyed (replace_tensor_to_optimizer).  Elementwise torch, no host synchronisation; a
    model without an opacity group (or optimizer) just gets the new tensor."""
    fn = "reset_opacity"
    old = g._opacity
    _check(old, "_opacity", fn)
    opacity = torch.sigmoid(old)
    x = torch.min(opacity, torch.ones_like(opacity) * 0.01)
    new = torch.log(x / (1 - x))  # utils/general_utils.inverse_sigmoid
    opt, groups = _groups(g, fn)
    group = groups.get("opacity")
    if group is None:
        g._opacity = nn.Parameter(new, requires_grad=old.requires_grad) if isinstance(old, nn.Parameter) else \
            new.requires_grad_(old.requires_grad)
        return
    p = nn.Parameter(new.requires_grad_(True))
    st = opt.state.get(old, None)
    if st is not None:
        if "exp_avg" in st:
            st["exp_avg"] = torch.zeros_like(new)
            st["exp_avg_sq"] = torch.zeros_like(new)
        del opt.state[old]
        opt.state[p] = st
    group["params"][0] = p
    g._opacity = p
