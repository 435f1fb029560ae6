"""The model this package exists to train, for tests: the reference GaussianModel's RAW parameters behind its activations
(tests/densify_reference.Model: exp(_scaling), sigmoid(_opacity), normalize(_rotation), cat(_features_dc, _features_rest),
_semantics * mask), so that the rasterizer's operands are non-leaf tensors with autograd nodes between them and the parameters.

    make(dev, P, S, sh_degree, seed, ...)  a Model whose activations reproduce scene.make_scene(P, S, sh_degree, seed, ...)
    twin(model)                            a render.GaussianSet whose LEAVES are detached clones of the model's activated tensors
    chain(model, operand_grads)            operand gradients (the twin's) pushed through the activations to the raw parameters

The operand-leaf path (the twin) is held against the oracle and float64 by the rest of the suite; `chain` composes it with torch's
own activation backward.  The same kernels see the same operands in the model and in its twin, and torch's activation backward
sees the same gradients in the model's graph and in `chain`: the raw-parameter gradients must agree bit for bit."""
import numpy as np
import torch
from torch import nn

from tests import densify_reference as ref

RAW = tuple(attr for _, attr in ref.PARAMS)
# operand name -> (the twin's leaf, the raw parameters behind it)
OPERANDS = {"xyz": ("_xyz", ("_xyz",)), "scaling": ("_scaling", ("_scaling",)), "rotation": ("_rotation", ("_rotation",)),
            "opacity": ("_opacity", ("_opacity",)), "features": ("_features", ("_features_dc", "_features_rest")),
            "semantics": ("_semantics", ("_semantics",))}


class Model(ref.Model):
    """densify_reference.Model plus the one accessor render() reads under compute_cov3D_python (scene/gaussian_model.py:126-127:
    the covariance is built from the activated scales and the RAW quaternions, normalised inside)."""

    def get_covariance(self, scaling_modifier=1.0):
        from goi_hyperplane_amd.render import covariance_from_scaling_rotation
        return covariance_from_scaling_rotation(self.get_scaling, scaling_modifier, self._rotation)


def make(dev, P, S=16, sh_degree=3, seed=0, rotation_norm=(0.5, 2.0), **scene_kwargs):
    """Raw parameters whose activations reproduce make_scene(P, S, sh_degree, seed, **scene_kwargs): _scaling = log(scales),
    _opacity = logit(opacity clipped to [1e-4, 1 - 1e-4]), _features_dc / _features_rest split from shs, and _rotation NOT of
    unit norm: every row scaled by a seeded factor in rotation_norm, so that normalize has a non-trivial Jacobian
    (rotation_norm=None: the scene's unit quaternions as they are)."""
    from goi_hyperplane_amd.scene import make_scene
    sc = make_scene(P, S=S, sh_degree=sh_degree, seed=seed, **scene_kwargs)
    m = Model()
    m.active_sh_degree = sh_degree
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)  # noqa: E731
    op = np.clip(sc.opacities, 1e-4, 1 - 1e-4)
    rot = sc.rotations
    if rotation_norm is not None:
        lo, hi = rotation_norm
        rot = rot * np.random.default_rng(seed + 77).uniform(lo, hi, size=(P, 1)).astype(np.float32)
    raw = {"_xyz": t(sc.means3D), "_scaling": torch.log(t(sc.scales)), "_rotation": t(rot),
           "_opacity": t(np.log(op / (1 - op))), "_features_dc": t(sc.shs[:, :1]), "_features_rest": t(sc.shs[:, 1:]),
           "_semantics": t(sc.semantics)}
    for attr, v in raw.items():
        setattr(m, attr, nn.Parameter(v.contiguous()))
    m.xyz_gradient_accum = torch.zeros(P, 1, device=dev)
    m.denom = torch.zeros(P, 1, device=dev)
    m.max_radii2D = torch.zeros(P, device=dev)
    return m


def raw_parameters(model, trainable_only=True):
    """{attribute: parameter} in densify_reference.PARAMS order"""
    return {a: getattr(model, a) for a in RAW if getattr(model, a).requires_grad or not trainable_only}


def set_trainable(model, *attrs):
    """only `attrs` keep requires_grad (none given: every raw parameter trains)"""
    for a in RAW:
        getattr(model, a).requires_grad_(not attrs or a in attrs)
    return model


def _operands(model, raw_rotation=False):
    return {"xyz": model.get_xyz, "scaling": model.get_scaling, "rotation": model._rotation if raw_rotation else model.get_rotation,
            "opacity": model.get_opacity, "features": model.get_features, "semantics": model.get_semantics}


def twin(model, raw_rotation=False):
    """A GaussianSet whose leaf parameters are detached clones of the model's activated tensors (get_xyz, get_scaling,
    get_rotation, get_features, get_opacity, get_semantics -- the semantic mask applied, none set on the twin); a leaf is
    trainable iff a raw parameter behind it is.  raw_rotation: the rotation leaf is the raw `_rotation` (what
    get_covariance reads under compute_cov3D_python)."""
    from goi_hyperplane_amd.render import GaussianSet
    with torch.no_grad():
        o = {k: v.detach().clone() for k, v in _operands(model, raw_rotation).items()}
    pc = GaussianSet(o["xyz"], o["scaling"], o["rotation"], o["opacity"], o["features"], o["semantics"],
                     sh_degree=model.active_sh_degree, max_sh_degree=model.max_sh_degree)
    for leaf, raws in OPERANDS.values():
        getattr(pc, leaf).requires_grad_(any(getattr(model, a).requires_grad for a in raws))
    return pc


def twin_gradients(pc):
    """{operand name: .grad of the twin's leaf (None where it has none)}: what `chain` takes"""
    return {k: getattr(pc, leaf).grad for k, (leaf, _raws) in OPERANDS.items()}


def chain(model, operand_grads, raw_rotation=False):
    """{raw attribute: gradient or None}: the activations recomputed from the raw parameters, and `operand_grads` ({operand name:
    gradient}; a missing or None entry contributes nothing) pushed through them with ONE torch.autograd.grad."""
    params = raw_parameters(model)
    ops = _operands(model, raw_rotation)
    pairs = [(ops[k], g) for k, g in operand_grads.items() if g is not None and ops[k].requires_grad]
    out = dict.fromkeys(RAW)
    if pairs and params:
        got = torch.autograd.grad([a for a, _g in pairs], list(params.values()), [g.view_as(a) for a, g in pairs], allow_unused=True)
        out.update(zip(params, got))
    return out
