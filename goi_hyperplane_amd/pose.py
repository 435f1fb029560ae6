"""Pose gradients of a selection of Gaussians and of the camera from ONE backward (csrc/pose.hip): the inverse
of goi_hyperplane_amd.edit.  edit.transform moves, turns and resizes a selected object; given a loss this module says which way.

The twist tau = (omega[3], t[3], sigma) applies the similarity T(tau) to the selected rows,

    x' = p + t + e^sigma Exp(omega) (x - p),   r' = q(omega) (x) r,   l' = l + sigma,   c'_l = D_l(Exp(omega)) c_l,

T(0) the identity.  After a backward, dL/d_xyz, dL/d_rotation, dL/d_scaling and dL/d_features_rest lie in the .grad tensors; by
the chain rule the gradient with respect to tau is one reduction of those rows over the selection, with d = x - p:

    dL/dt     = sum g_x
    dL/dsigma = sum [ g_x . d + (g_l0 + g_l1 + g_l2) ]
    dL/domega = sum [ d x g_x  +  1/2 (-g_w v + w g_v + v x g_v)  +  (sum_ch g_c[:, ch]^T G_k c[:, ch])_{k = x, y, z} ]

with r = (w, v), g_r = (g_w, g_v) on the RAW quaternion (the product acts on it, so nothing is normalised) and G_k the generators
of the real-SH rotation matrices of this project's basis (sh_generators).  _features_dc, _opacity and _semantics do not move under
T and contribute nothing.

    gradient(g, selection=None, *, pivot="centroid", invert=False, grads=None)   {"rotation", "translation", "log_scale", "count"}
    camera_gradient(g, *, pivot="origin", grads=None)                            {"rotation", "translation"}
    fit(g, selection, closure, *, iterations, lr_rotation, lr_translation, ...)  the host loop: Adam on tau, edit.transform in place
    sh_generators(degree=3)       float64 [3, n, n]
    twist_rotation(omega)         float64 [3, 3], Rodrigues

One kernel launch and a one-workgroup final pass (plus the two of edit.selection_bounds for a derived pivot); no host
synchronisation, no float atomics: the same bits on every run.  Per selected row every piece is formed in fp32, one rounding per
operation in the order tests/pose_reference.py writes down, converted to float64 and summed in float64 in a fixed order.  fp32
tensors on a ROCm GPU only; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib, edit
from ._lib import check, ptr, stream, workspace

GRADS = ("_xyz", "_rotation", "_scaling", "_features_rest")
_ZERO = 1e-13  # below this a generator's entry is one of the basis' structural zeros (the solve leaves a few 1e-16 there)
NONZEROS = (18, 18, 12)  # of G_x, G_y, G_z over bands 1..3: a property of the basis, compiled into csrc/pose.hip


# ---- host mathematics (float64) ---------------------------------------------------------------------------------------------
def _cross_matrix(k):
    K = np.zeros((3, 3), dtype=np.float64)
    a, b = (k + 1) % 3, (k + 2) % 3
    K[b, a], K[a, b] = 1.0, -1.0
    return K


_GENERATORS = []


def sh_generators(degree=3):
    """float64 [3, n, n], n = (degree + 1)^2: G_k = d/dtheta D(Exp(theta e_k)) at theta = 0 for k = x, y, z, D = edit.sh_rotation.
    Block diagonal over the bands, skew, [G_x, G_y] = G_z; the band-0 row and column are zero.  Formed once from the sampling
    edit.sh_rotation uses: within a band D_l = pinv(Y_l) (monomials(d R) coeff_l), the monomials are polynomials in R, and their
    derivative along R = I + theta [e_k]_x is taken by a complex step (exact to rounding: nothing is subtracted).  The basis'
    structural zeros are stored as exact zeros."""
    if degree not in (0, 1, 2, 3):
        raise ValueError(f"sh_generators: degree must be 0..3, got {degree}")
    if not _GENERATORS:
        d, solvers = edit._sampling()
        h = 1e-30
        G = np.zeros((3, 16, 16), dtype=np.float64)
        for k in range(3):
            mono = edit._monomials(d @ (np.eye(3) + 1j * h * _cross_matrix(k)))
            for l in (1, 2, 3):
                a, b = l * l, (l + 1) * (l + 1)
                pinv, coeff = solvers[l - 1]
                G[k, a:b, a:b] = pinv @ ((mono[l - 1].imag / h) @ coeff)
        G[np.abs(G) < _ZERO] = 0.0
        if tuple(int(np.count_nonzero(G[k])) for k in range(3)) != NONZEROS:
            raise RuntimeError("sh_generators: the generators do not have the sparsity pattern csrc/pose.hip compiles in")
        _GENERATORS.append(G)
    n = (degree + 1) ** 2
    return _GENERATORS[0][:, :n, :n].copy()


def generator_entries(k, M=16):
    """[(i, j)] of the non-zero entries of G_k within the first M coefficients, row-major, as indices into _features_rest's
    M - 1 rows (coefficient 1 is row 0): the order in which csrc/pose.hip takes its 48 values and adds the colour terms"""
    G = sh_generators(3)[k]
    return [(int(i) - 1, int(j) - 1) for i, j in zip(*np.nonzero(G)) if i < M and j < M]


def twist_rotation(omega):
    """float64 [3, 3]: Exp(omega) = I + (sin th / th) K + (1 - cos th) / th^2 K^2 with K = [omega]_x, th = |omega| (Rodrigues;
    1 - cos th as 2 sin^2(th / 2), which keeps its digits for small th).  Exactly the identity at omega = 0."""
    w = edit._host_array(omega, "omega", "twist_rotation")
    if w.shape != (3,):
        raise ValueError(f"twist_rotation: omega must be three numbers, got shape {w.shape}")
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    half = math.sin(0.5 * th) / th
    return np.eye(3) + (math.sin(th) / th) * K + (2.0 * half * half) * (K @ K)


_PACKED = []


def _packed_generators():
    """the 48 non-zero generator values as the C array the kernel takes by value: G_x, G_y, G_z, row-major within each"""
    if not _PACKED:
        G = sh_generators(3)
        vals = [float(G[k][i + 1, j + 1]) for k in range(3) for i, j in generator_entries(k)]
        _PACKED.append((ctypes.c_float * 48)(*vals))
    return _PACKED[0]


# ---- the reduction ----------------------------------------------------------------------------------------------------------
def _collect_grads(g, grads, fn):
    if grads is None:
        found = {attr: getattr(g, attr).grad for attr in GRADS}
    else:
        if not isinstance(grads, dict) or set(grads) != set(GRADS):
            raise ValueError(f"{fn}: grads must be a dict with the keys {GRADS}")
        found = dict(grads)
    if all(v is None for v in found.values()):
        raise ValueError(f"{fn}: none of {GRADS} has a gradient; run a backward first (loss.backward(), or pass grads=)")
    return found


def _launch(g, selection, pivot, invert, grads, fn):
    """(out float64 [7] = omega | t | sigma, count int32 [1]), both on the device"""
    kind, pv = edit._pivot(pivot, fn)
    xyz = g._xyz
    edit._check_tensor(xyz, "_xyz", fn)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{fn}: _xyz has shape {tuple(xyz.shape)}, expected [P, 3]")
    P, dev = int(xyz.shape[0]), xyz.device
    params = {"_xyz": xyz}
    for attr in ("_rotation", "_scaling"):
        edit._check_tensor(getattr(g, attr), attr, fn, (P,) + edit._ROW[attr])
        params[attr] = getattr(g, attr)
    rest = g._features_rest
    edit._check_tensor(rest, "_features_rest", fn)
    if rest.dim() != 3 or rest.shape[0] != P or rest.shape[2] != 3 or int(rest.shape[1]) + 1 not in (1, 4, 9, 16):
        raise ValueError(f"{fn}: _features_rest has shape {tuple(rest.shape)}, expected [{P}, M - 1, 3] with M in (1, 4, 9, 16)")
    params["_features_rest"] = rest
    M = int(rest.shape[1]) + 1
    found = _collect_grads(g, grads, fn)
    edit._check_selection(selection, P, dev, fn)
    tensors = list(params.items())
    for attr in GRADS:
        if found[attr] is not None:
            edit._check_tensor(found[attr], f"the gradient of {attr}", fn, tuple(params[attr].shape))
            tensors.append((f"the gradient of {attr}", found[attr]))
    if kind == "device":
        tensors.append(("pivot", pv))
    edit._check_device(tensors, dev, fn)
    sel = None if selection is None else selection.contiguous()
    if M == 1:
        found["_features_rest"] = None  # [P, 0, 3]: nothing to turn
        if all(v is None for v in found.values()):
            raise ValueError(f"{fn}: none of {GRADS} has a gradient; run a backward first (loss.backward(), or pass grads=)")

    lib = _lib.load()
    nbytes = int(lib.goi_pose_gradient_workspace_bytes(P))
    if nbytes == 0:
        raise ValueError(f"{fn}: P = {P} is out of range (P < 2^31)")
    pivot_dev, host_pivot = None, np.zeros(3)
    if kind == "derived":
        _count, bounds = edit._bounds_launch(xyz.detach(), sel, invert, dev)
        pivot_dev = bounds[6:9] if pv == "centroid" else bounds[9:12]
    elif kind == "device":
        pivot_dev = pv.detach()
    else:
        host_pivot = pv
    ws = workspace(nbytes, dev)
    out = torch.empty(7, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    gp = {attr: None if found[attr] is None else found[attr].detach() for attr in GRADS}
    with torch.cuda.device(dev):
        check(lib.goi_pose_gradient(P, M, ptr(sel), 1 if invert else 0,
                                    ptr(xyz.detach()) if gp["_xyz"] is not None else None,
                                    ptr(params["_rotation"].detach()) if gp["_rotation"] is not None else None,
                                    ptr(rest.detach()) if gp["_features_rest"] is not None else None,
                                    ptr(gp["_xyz"]), ptr(gp["_rotation"]), ptr(gp["_scaling"]), ptr(gp["_features_rest"]),
                                    _packed_generators(), (ctypes.c_float * 3)(*[float(v) for v in host_pivot]), ptr(pivot_dev),
                                    ptr(count), ptr(out), ptr(ws), stream(dev)), ValueError)
    return out, count


def gradient(g, selection=None, *, pivot="centroid", invert=False, grads=None):
    """dL/dtau of moving the selected Gaussians of `g` by T(tau) about `pivot`, at tau = 0 (see the module docstring):
    {"rotation": float64 [3] (dL/domega), "translation": float64 [3] (dL/dt), "log_scale": float64 [] (dL/dsigma),
    "count": int32 [1] (selected rows)}, all on the device, without a read-back.

    `g`, selection, invert and pivot as in edit.transform: pivot "centroid" / "center" (of the selection, through
    edit.selection_bounds, read from device memory), "origin", three host numbers or a device tensor [3].  grads: None takes the
    .grad of _xyz, _rotation, _scaling and _features_rest as a backward left them; or a dict with those four keys (for
    torch.autograd.grad).  A None entry was not trained: its terms are omitted and its parameter is not read.  All four None
    raises a ValueError.  Nothing is written, so a semantic mask set on the model is not refused.  An empty selection gives
    zeros and count 0."""
    out, count = _launch(g, selection, pivot, invert, grads, "gradient")
    return {"rotation": out[0:3], "translation": out[3:6], "log_scale": out[6], "count": count}


def camera_gradient(g, *, pivot="origin", grads=None):
    """dL/d(omega, t) of moving the CAMERA by T(tau) about `pivot` (edit.transform_camera(camera, rotation=twist_rotation(omega),
    translation=t, pivot=pivot)), at tau = 0: {"rotation": float64 [3], "translation": float64 [3]} on the device.  Since
    render(T model, T camera) = render(model, camera) and T(tau)^-1 = T(-tau) to first order about the same pivot, it is MINUS
    the whole-model gradient.  Pass the camera's centre as `pivot` for a twist about the camera itself.

    This holds for omega and t, and for a loss on the image, semantics or alpha maps.  Under sigma the depth map scales with the
    model, so no log_scale is returned, and a loss that reads the DEPTH map is the caller's responsibility."""
    out, _count = _launch(g, None, pivot, False, grads, "camera_gradient")
    return {"rotation": -out[0:3], "translation": -out[3:6]}


# ---- the host loop ----------------------------------------------------------------------------------------------------------
def fit(g, selection, closure, *, iterations, lr_rotation, lr_translation, lr_log_scale=0.0, invert=False, moments=True):
    """Snaps the selected Gaussians onto what a loss asks for: `iterations` Adam steps on the twist, each applied in place.

    closure() zeroes the gradients, renders, calls loss.backward() and returns the loss (a tensor).  Per iteration: gradient()
    about the selection's current centroid; ONE read-back of the seven numbers, the centroid and the loss; an Adam step on tau in
    float64 on the host (a component whose learning rate is 0 is frozen: it gets no rotation / a scale of exactly 1); then
    edit.transform(g, selection, rotation=twist_rotation(d_omega), translation=d_t, scale=exp(d_sigma), pivot=<that centroid>,
    invert=invert, moments=moments).

    Returns (R, t, s, history): the composite similarity x' = s R x + t of all the steps in float64, and history = {"loss": the
    closure's value before each step, "steps": [{"rotation", "translation", "scale", "pivot"}] as handed to edit.transform}."""
    fn = "fit"
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"{fn}: iterations must be >= 0")
    lr = np.array([lr_rotation] * 3 + [lr_translation] * 3 + [lr_log_scale], dtype=np.float64)
    if not np.all(np.isfinite(lr)) or np.any(lr < 0):
        raise ValueError(f"{fn}: learning rates must be finite and >= 0")
    b1, b2, eps = 0.9, 0.999, 1e-8  # Adam's defaults
    m, v = np.zeros(7), np.zeros(7)
    R_all, t_all, s_all = np.eye(3), np.zeros(3), 1.0
    history = {"loss": [], "steps": []}
    for it in range(1, iterations + 1):
        loss = closure()
        bounds = edit.selection_bounds(g._xyz.detach(), selection, invert=invert)
        out, _count = _launch(g, selection, bounds["centroid"], invert, None, fn)
        host = torch.cat([out, bounds["centroid"].double(), loss.detach().double().reshape(1)]).cpu().numpy()
        grad, c = host[:7], host[7:10]
        history["loss"].append(float(host[10]))
        m = b1 * m + (1 - b1) * grad
        v = b2 * v + (1 - b2) * grad * grad
        step = -lr * (m / (1 - b1 ** it)) / (np.sqrt(v / (1 - b2 ** it)) + eps)
        R = twist_rotation(step[0:3])
        s = math.exp(step[6])
        kw = dict(rotation=R if lr_rotation > 0 else None, translation=step[3:6], scale=s, pivot=c)
        edit.transform(g, selection, invert=invert, moments=moments, **kw)
        history["steps"].append(kw)
        R_all, t_all, s_all = R @ R_all, c + step[3:6] + s * (R @ (t_all - c)), s * s_all
    return R_all, t_all, s_all, history
