"""Densification semantics in plain torch, device-agnostic: what goi_hyperplane_amd.densify must compute, formulated
directly as the final layout

    [originals not split, not pruned] [clones not pruned] [first children not pruned] [second children not pruned]

rather than as the reference's sequence of cat / prune steps (scene/gaussian_model.py:291-513).  Every elementwise op
runs on a tensor of the same shape and row order as in the reference's sequence (exp over the post-clone rows, the
prune tests over the pre-prune rows), so that torch's elementwise kernels see the same operands as in the reference.
tests/test_densify_cpu.py holds it bit-exact to the reference's own methods on the CPU (tests/golden/ref_densify_pins.npz,
written by tests/golden/make_densify_golden.py); the GPU tests run it on the device as the comparison for the HIP path.
It has the package's documented differences from the reference: a parameter without an optimizer group (or optimizer
None) is still compacted / extended, a statistic that was never set up is left as it is by prune_points, reset_opacity
needs no optimizer state, and a model with _semantics_masks set is refused.

Also `Model` (the reference GaussianModel's attribute surface plus the accessors render() reads) and `make_model` (a
seeded model with a stepped optimizer whose derived values keep clear of the thresholds)."""
import math
import os

import torch
from torch import nn

PARAMS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("semantics", "_semantics"),
          ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))
ATTR = dict(PARAMS)
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")


class Model:
    """The reference GaussianModel's attributes with its activations, and the accessors render() reads."""

    def __init__(self):
        self.active_sh_degree = self.max_sh_degree = 3
        self.optimizer = None
        self.percent_dense = 0.01
        self._semantics_masks = None

    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: nn.functional.normalize(self._rotation))
    get_opacity = property(lambda self: torch.sigmoid(self._opacity))

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_semantics(self):
        return self._semantics if self._semantics_masks is None else self._semantics * self._semantics_masks

    def set_semantic_masks(self, masks=None):
        self._semantics_masks = None if masks is None else masks.unsqueeze(1)


def rotation_matrices(q):
    """[n, 3, 3] rotation of the raw quaternions q [n, 4] = (r, x, y, z), normalised first; fp32 elementwise ops in the
    order of utils/general_utils.build_rotation (squares summed left to right)"""
    n = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    u = q / n[:, None]
    r, x, y, z = u[:, 0], u[:, 1], u[:, 2], u[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=-1).reshape(-1, 3, 3)


def _groups(g):
    if getattr(g, "_semantics_masks", None) is not None:
        raise ValueError("the model has a semantic mask set")
    return {} if g.optimizer is None else {grp["name"]: grp for grp in g.optimizer.param_groups}


def _replace(g, name, new, moments):
    """model attribute + optimizer group of `name` -> `new`; moments: (exp_avg, exp_avg_sq) -> the state's new moments"""
    attr = ATTR[name]
    old = getattr(g, attr)
    group = _groups(g).get(name)
    if group is None:
        setattr(g, attr, nn.Parameter(new, requires_grad=old.requires_grad))
        return
    p = nn.Parameter(new.requires_grad_(True))
    st = g.optimizer.state.get(old, None)
    if st is not None:
        if "exp_avg" in st:
            st["exp_avg"], st["exp_avg_sq"] = moments(st["exp_avg"], st["exp_avg_sq"])
        del g.optimizer.state[old]
        g.optimizer.state[p] = st
    group["params"][0] = p
    setattr(g, attr, p)


@torch.no_grad()
def prune_points(g, mask):
    keep = ~mask
    for name, attr in PARAMS:
        _replace(g, name, getattr(g, attr).detach()[keep], lambda m, v: (m[keep], v[keep]))
    P = mask.shape[0]
    for name in STATS:
        t = getattr(g, name)
        if t.numel() == 0 and t.shape[0] != P:
            continue  # never set up (a model loaded from a .ply)
        setattr(g, name, t[keep])


@torch.no_grad()
def densify_and_prune(g, max_grad, min_opacity, extent, max_screen_size, generator=None, normal=None):
    """Returns {"kept", "clones", "children"}: the sizes K, C', S' of the first three blocks, and "samples_norm": the norms
    of the kept children's samples in their row order (first children, then second)."""
    if normal is None:
        def normal(mean, std):
            return torch.normal(mean=mean, std=std, generator=generator)
    _groups(g)
    dev = g._xyz.device
    raw = {attr: getattr(g, attr).detach() for _, attr in PARAMS}
    P = raw["_xyz"].shape[0]
    grad = g.xyz_gradient_accum / g.denom
    grad = torch.where(grad.isnan(), torch.zeros_like(grad), grad)
    thr_s = g.percent_dense * extent

    clone = (torch.linalg.vector_norm(grad, dim=-1) >= max_grad) & (torch.exp(raw["_scaling"]).max(dim=1).values <= thr_s)
    # the split decision sees the post-clone rows (exp over them); clones have a padded gradient of 0 and are never split
    scal_pc = torch.exp(torch.cat((raw["_scaling"], raw["_scaling"][clone])))[:P]
    split = (grad.reshape(-1) >= max_grad) & (scal_pc.max(dim=1).values > thr_s)
    n = int(split.sum())

    stds = scal_pc[split].repeat(2, 1)
    samples = normal(mean=torch.zeros((2 * n, 3), device=dev), std=stds)
    child = {attr: t[split].repeat(2, *([1] * (t.dim() - 1))) for attr, t in raw.items()}
    child["_xyz"] = torch.bmm(rotation_matrices(raw["_rotation"][split]).repeat(2, 1, 1),
                              samples.unsqueeze(-1)).squeeze(-1) + raw["_xyz"][split].repeat(2, 1)
    child["_scaling"] = torch.log(scal_pc[split].repeat(2, 1) / (0.8 * 2))

    # the pre-prune rows: originals not split, clones, children; the final prune test over all of them
    rows = {attr: torch.cat((t[~split], t[clone], child[attr])) for attr, t in raw.items()}
    n_orig, n_clone = int((~split).sum()), int(clone.sum())
    prune = (torch.sigmoid(rows["_opacity"]) < min_opacity).reshape(-1)
    if max_screen_size:
        radii = torch.zeros(rows["_xyz"].shape[0], device=dev)  # max_radii2D was zeroed before the reference tests it
        prune = prune | (radii > max_screen_size) | (torch.exp(rows["_scaling"]).max(dim=1).values > 0.1 * extent)
    keep = ~prune

    for name, attr in PARAMS:
        def moments(m, v, attr=attr):
            z = torch.zeros((n_clone + 2 * n,) + tuple(m.shape[1:]), dtype=m.dtype, device=dev)
            return torch.cat((m[~split], z))[keep], torch.cat((v[~split], z))[keep]
        _replace(g, name, rows[attr][keep], moments)
    P_new = g._xyz.shape[0]
    g.xyz_gradient_accum = torch.zeros((P_new, 1), device=dev)
    g.denom = torch.zeros((P_new, 1), device=dev)
    g.max_radii2D = torch.zeros((P_new,), device=dev)
    kc = keep[n_orig + n_clone:]
    return {"kept": int(keep[:n_orig].sum()), "clones": int(keep[n_orig:n_orig + n_clone].sum()),
            "children": int(kc[:n].sum()), "samples_norm": samples.norm(dim=1)[kc]}


@torch.no_grad()
def add_densification_stats(g, viewspace_point_tensor, update_filter):
    norms = torch.linalg.vector_norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1, keepdim=True)
    g.xyz_gradient_accum[update_filter] = g.xyz_gradient_accum[update_filter] + norms
    g.denom[update_filter] = g.denom[update_filter] + 1


@torch.no_grad()
def reset_opacity(g):
    o = torch.sigmoid(g._opacity)
    x = torch.min(o, torch.ones_like(o) * 0.01)
    _replace(g, "opacity", torch.log(x / (1 - x)), lambda m, v: (torch.zeros_like(m), torch.zeros_like(v)))


# ---- seeded models ------------------------------------------------------------------------------------------------------

def _nudge(x, tests, margin=1e-5, step=3e-5):
    """moves the raw values whose derived value f(x) lies within `margin` (relative) of its threshold a little away"""
    for _ in range(8):
        bad = torch.zeros_like(x, dtype=torch.bool)
        for f, thr in tests:
            if thr != 0 and math.isfinite(thr):
                bad |= (f(x) - thr).abs() <= margin * abs(thr)
        if not bool(bad.any()):
            break
        x = torch.where(bad, x + step * (1 + x.abs()), x)
    return x


def make_model(P, device, seed=0, S=16, M=16, optimizer="adam", steps=2, max_grad=2e-4, percent_dense=0.01, extent=4.0,
               min_opacity=0.1, denom_zero=0.05, scale_std=0.9):
    """A seeded reference-style model: about half of the Gaussians above the split scale, gradients spread around
    max_grad, some 0/0 and x/0 statistics, some opacities below min_opacity; the derived values (gradient, scales,
    children's scales, sigmoid(opacity)) keep more than 1e-5 relative away from the thresholds.  optimizer: "adam",
    "fused", "partial" (f_dc and f_rest only, as finetune_sh_setup builds it) or None; `steps` Adam steps on seeded
    gradients (0: the state was never stepped).  scale_std: spread of the log-scales around log(percent_dense * extent)."""
    gen = torch.Generator().manual_seed(seed)

    def r(*shape):
        return torch.randn(*shape, generator=gen)

    thr_s, big = percent_dense * extent, 0.1 * extent
    m = Model()
    m.percent_dense = percent_dense
    scaling = _nudge(math.log(thr_s) + scale_std * r(P, 3),
                     [(torch.exp, thr_s), (torch.exp, big), (lambda s: torch.exp(torch.log(torch.exp(s) / 1.6)), big)])
    opacity = _nudge(1.5 * r(P, 1), [(torch.sigmoid, min_opacity)])
    denom = torch.randint(1, 6, (P, 1), generator=gen).float()
    zero = torch.rand(P, 1, generator=gen) < denom_zero
    accum = torch.rand(P, 1, generator=gen) * (2.5 * max_grad) * torch.where(denom > 0, denom, torch.ones_like(denom))
    accum = _nudge(accum, [(lambda a: a / torch.where(denom > 0, denom, torch.ones_like(denom)), max_grad)], step=1e-8)
    denom = torch.where(zero, torch.zeros_like(denom), denom)
    accum = torch.where(zero & (torch.rand(P, 1, generator=gen) < 0.5), torch.zeros_like(accum), accum)  # 0/0 and x/0
    tensors = {"_xyz": r(P, 3), "_features_dc": r(P, 1, 3), "_features_rest": 0.3 * r(P, M - 1, 3), "_semantics": r(P, S),
               "_opacity": opacity, "_scaling": scaling, "_rotation": r(P, 4)}
    for attr, t in tensors.items():
        setattr(m, attr, nn.Parameter(t.to(device).contiguous()))
    m.xyz_gradient_accum = accum.to(device)
    m.denom = denom.to(device)
    m.max_radii2D = (torch.rand(P, generator=gen) * 40).to(device)
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "semantics": 1e-3, "opacity": 0.05, "scaling": 5e-3,
           "rotation": 1e-3}
    if optimizer is None:
        return m
    names = ("f_dc", "f_rest") if optimizer == "partial" else tuple(lrs)
    groups = [{"params": [getattr(m, ATTR[n])], "lr": lrs[n], "name": n} for n in names]
    if optimizer == "fused":
        from goi_hyperplane_amd.optim import FusedAdam
        m.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
    else:
        m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for _ in range(steps):
        for n in names:
            p = getattr(m, ATTR[n])
            p.grad = r(*p.shape).to(device)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    return m


# ---- the pins of the reference's own methods (tests/golden/ref_densify_pins.npz, make_densify_golden.py) ---------------

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_densify_pins.npz")


def pins():
    import numpy as np
    return np.load(PINS)


def pins_model(d, device, fused=False):
    """the pinned input model on `device` with its 7-group optimizer state (torch.optim.Adam, or FusedAdam)"""
    m = Model()
    m.percent_dense = float(d["percent_dense"])
    for _, attr in PARAMS:
        setattr(m, attr, nn.Parameter(torch.from_numpy(d[f"in{attr}"].copy()).to(device)))
    for name in STATS:
        setattr(m, name, torch.from_numpy(d[f"in_{name}"].copy()).to(device))
    groups = [{"params": [getattr(m, attr)], "lr": 1e-3, "name": name} for name, attr in PARAMS]
    if fused:
        from goi_hyperplane_amd.optim import FusedAdam
        m.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
    else:
        m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for name, attr in PARAMS:
        m.optimizer.state[getattr(m, attr)] = {
            "step": torch.tensor(float(d[f"in_{name}_step"])),
            "exp_avg": torch.from_numpy(d[f"in_{name}_exp_avg"].copy()).to(device),
            "exp_avg_sq": torch.from_numpy(d[f"in_{name}_exp_avg_sq"].copy()).to(device)}
    return m


def pinned_outputs(d, case):
    """{key: array} of a case's pinned parameters, moments, steps and statistics (the keys make_densify_golden writes)"""
    out = {attr: d[f"{case}{attr}"] for _, attr in PARAMS}
    for name, _ in PARAMS:
        for k in ("exp_avg", "exp_avg_sq", "step"):
            out[f"{name}_{k}"] = d[f"{case}_{name}_{k}"]
    for name in STATS:
        out[name] = d[f"{case}_{name}"]
    return out


def model_outputs(m):
    """the same keys as pinned_outputs, from a model (tensors on any device)"""
    out = {attr: getattr(m, attr).detach().cpu().numpy() for _, attr in PARAMS}
    for name, attr in PARAMS:
        st = m.optimizer.state[getattr(m, attr)]
        out[f"{name}_exp_avg"] = st["exp_avg"].cpu().numpy()
        out[f"{name}_exp_avg_sq"] = st["exp_avg_sq"].cpu().numpy()
        out[f"{name}_step"] = float(st["step"])
    for name in STATS:
        out[name] = getattr(m, name).cpu().numpy()
    return out
