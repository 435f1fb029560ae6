"""Rigid edits of a selection of Gaussians on the device (csrc/edit.hip): moving, turning and resizing the selected object,

    x' = p + t + s R (x - p),

applied IN PLACE to the selected rows of a model.  The reference's viewer can only translate (gui/main_edit.py:1512-1548,
obj_move: `gaussians._xyz[~nograd_mask] += dir * 0.1`); turning or resizing an object needs its covariances turned and its
view-dependent colour (SH bands 1..3) rotated with it, or its highlights end up on the wrong side.

    transform(g, selection=None, *, rotation=None, translation=None, scale=1.0, pivot="centroid", invert=False, moments=True)
    move(g, selection, direction)                     the reference's obj_move, bit for bit
    selection_bounds(xyz, selection=None, invert=False)   count, lo, hi, centroid, center -- device tensors, no read-back
    sh_rotation(R, degree=3)                          the real-SH rotation matrices of this project's basis, float64
    transform_camera(camera, ...)                     the same similarity applied to a scene.Camera

`g` is any object with the reference GaussianModel's attributes, exactly as densify.py takes them.  Per selected Gaussian:
_xyz as above; _rotation (raw, (w, x, y, z)) becomes q_R (x) r -- the norm is preserved, so the activated covariance is
R Sigma R^T; _scaling (raw log) gets + log s; every stored band l = 1..3 of _features_rest [P, M-1, 3] (M in 1, 4, 9, 16) is
multiplied by its real-SH rotation matrix D_l per channel, whatever active_sh_degree says.  _features_dc, _opacity, _semantics,
the densification statistics and every unselected row stay bit-unchanged.  max_radii2D goes stale under s != 1 (it is the
screen-space radius densification last saw; the next densification interval refreshes it).

Arithmetic: R, q_R, t, p, s, log s and the D_l are formed on the host in float64, rounded to fp32 once and handed to the kernel by
value; the kernel rounds once per operation in the order tests/edit_reference.py writes down.  A pure translation (no rotation,
scale 1) is the single add x + t, with no pivot involved.

Adam state (torch.optim.Adam or FusedAdam, groups named as in densify.py; optimizer None, a partial group list and state never
stepped are all fine): under a rotation the first moments are vectors and turn with their parameter -- exp_avg of xyz gets R m,
of rotation q_R (x) m, of f_rest D_l m; no translation, pivot or scale is applied to a moment (under s != 1 the moments keep their
magnitudes).  exp_avg_sq holds per-component magnitudes, has no exact image under a rotation and stays bit-unchanged, like
`step` and every other group.  moments=False leaves the state alone.

pivot "centroid" / "center" launches selection_bounds and the transform kernel reads p from device memory: the call never
synchronises.  Every tensor written has its version counter bumped (the kernels write through raw pointers), so the geometry
cache (rasterizer.set_geometry_cache) never reblends a camera's cached geometry after an edit.  fp32 tensors on a ROCm GPU only;
there is no CPU fallback.  A mirror (det R < 0) is refused, not approximated.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib, densify
from ._lib import check, ptr, stream, workspace
from .render import SH_C0, SH_C1, SH_C2, SH_C3

_NO_CPU = "goi_hyperplane_amd.edit: tensors must live on a ROCm GPU; there is no CPU fallback"
_PIVOTS = ("centroid", "center", "origin")
_ROW = {"_xyz": (3,), "_rotation": (4,), "_scaling": (3,)}
ORTHO_TOL = 1e-6  # max |R^T R - I| a rotation matrix may have (an fp32 matrix has ~1e-7)
_N_DIRS = 64


# ---- host mathematics (float64) ---------------------------------------------------------------------------------------------
def _sh_basis(d, degree):
    """d [n, 3] unit -> [n, (degree+1)^2]: the basis of cuda_rasterizer/auxiliary.h (the constants and signs render.eval_sh uses)"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    b = [np.full_like(x, SH_C0)]
    if degree > 0:
        b += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
    if degree > 2:
        b += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
              SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
              SH_C3[6] * x * (xx - 3 * yy)]
    return np.stack(b, axis=1)


def _directions():
    """64 fixed, well spread unit vectors (a golden-angle spiral)"""
    k = np.arange(_N_DIRS, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / _N_DIRS
    r = np.sqrt(1.0 - z * z)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def sh_rotation(R, degree=3):
    """float64 [(degree+1)^2, (degree+1)^2], block diagonal (1, D_1 3x3, D_2 5x5, D_3 7x7): the coefficients c' = D c of the
    function rotated by R, sum_k c'_k Y_k(R d) = sum_k c_k Y_k(d), in this project's real SH basis.  D(R1 R2) = D(R1) D(R2).
    By sampling: within a band, Y_l(R^T d) = Y_l(d) D_l for every d, solved over 64 fixed directions (the bands' condition
    numbers are <= 1.6, so D is orthogonal to a few 1e-15); the basis at the rotated directions comes from their degree-l
    monomials through coefficients fitted once."""
    if degree not in (0, 1, 2, 3):
        raise ValueError(f"sh_rotation: degree must be 0..3, got {degree}")
    return _sh_rotation(_rotation_matrix(R, "sh_rotation"), degree)


def _sh_rotation(R, degree):
    """sh_rotation of a float64 rotation matrix that has been checked"""
    d, solvers = _sampling()
    mono = _monomials(d @ R)
    n = (degree + 1) ** 2
    D = np.zeros((n, n), dtype=np.float64)
    D[0, 0] = 1.0  # band 0 is a constant
    for l in range(1, degree + 1):
        a, b = l * l, (l + 1) * (l + 1)
        pinv, coeff = solvers[l - 1]
        D[a:b, a:b] = pinv @ (mono[l - 1] @ coeff)
    return D


# the monomials of degree 2 (xx yy zz xy yz xz) and 3 (xxx yyy zzz xxy xxz yyx yyz zzx zzy xyz) as products of columns
_DEG2 = (np.array([0, 1, 2, 0, 1, 0]), np.array([0, 1, 2, 1, 2, 2]))
_DEG3 = (np.array([0, 1, 2, 0, 0, 1, 1, 2, 2, 3]), np.array([0, 1, 2, 1, 2, 0, 2, 0, 1, 2]))  # (degree-2 monomial, axis)


def _monomials(d):
    """d [n, 3] -> ([n, 3], [n, 6], [n, 10]): band l of the basis is a linear map of the degree-l monomials"""
    m2 = d[:, _DEG2[0]] * d[:, _DEG2[1]]
    return d, m2, m2[:, _DEG3[0]] * d[:, _DEG3[1]]


_SAMPLING = []


def _sampling():
    """(the fixed directions, [(pinv(Y_l(directions)), the coefficients of Y_l in the degree-l monomials) for l = 1..3]): the same
    for every rotation, formed once.  A call then costs three small products instead of the basis at 64 directions."""
    if not _SAMPLING:
        d = _directions()
        Y = _sh_basis(d, 3)
        mono = _monomials(d)
        solvers = []
        for l in (1, 2, 3):
            Yl = Y[:, l * l:(l + 1) * (l + 1)]
            solvers.append((np.linalg.pinv(Yl), np.linalg.lstsq(mono[l - 1], Yl, rcond=None)[0]))
        _SAMPLING.extend((d, solvers))
    return _SAMPLING


def _quat_to_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def _matrix_to_quat(R):
    """(w, x, y, z), unit, w >= 0 where it can be chosen: the branch with the largest pivot"""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def _host_array(v, what, fn):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: {what} must be numbers") from None
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{fn}: {what} must be finite")
    return a


def _rotation_matrix(rotation, fn):
    """float64 [3, 3] from a 3x3 matrix or a (w, x, y, z) quaternion; None is the identity.  A matrix must be a proper rotation
    to ORTHO_TOL; it is then moved to the nearest exact rotation (polar factor), so that q, R and the D_l describe one rotation."""
    if rotation is None:
        return np.eye(3)
    a = _host_array(rotation, "rotation", fn)
    if a.shape == (4,):
        n = np.linalg.norm(a)
        if not n > 0:
            raise ValueError(f"{fn}: the rotation quaternion is zero")
        return _quat_to_matrix(a / n)
    if a.shape != (3, 3):
        raise ValueError(f"{fn}: rotation must be a 3x3 matrix or a (w, x, y, z) quaternion, got shape {a.shape}")
    err = float(np.abs(a.T @ a - np.eye(3)).max())
    if err > ORTHO_TOL:
        raise ValueError(f"{fn}: rotation is not orthonormal (max |R^T R - I| = {err:.3g} > {ORTHO_TOL})")
    if np.linalg.det(a) < 0:
        raise ValueError(f"{fn}: rotation has determinant -1: a mirror is not a rotation and is refused")
    u, _, vt = np.linalg.svd(a)
    return u @ vt


class Similarity:
    """The host side of one edit, float64: R [3,3], q (w, x, y, z), t [3], s, and whether a rotation / a scale was asked for."""

    def __init__(self, rotation=None, translation=None, scale=1.0, fn="transform"):
        self.R = _rotation_matrix(rotation, fn)
        self.rotate = rotation is not None
        self.q = _matrix_to_quat(self.R)
        t = np.zeros(3) if translation is None else _host_array(translation, "translation", fn)
        if t.shape != (3,):
            raise ValueError(f"{fn}: translation must be three numbers, got shape {t.shape}")
        self.t = t
        try:
            s = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: scale must be a number") from None
        if not math.isfinite(s) or s <= 0:
            raise ValueError(f"{fn}: scale must be finite and > 0, got {scale}")
        self.s = s
        self.scale = s != 1.0

    def struct(self, pivot):
        """The GoiEditTransform of this edit: everything rounded to fp32 once."""
        D = _sh_rotation(self.R, 3)
        t = _lib.GoiEditTransform()
        t.R[:] = self.R.reshape(-1).tolist()
        t.q[:] = self.q.tolist()
        t.t[:] = self.t.tolist()
        t.pivot[:] = [float(v) for v in pivot]
        t.s, t.log_s = self.s, math.log(self.s)
        t.flags = (_lib.EDIT_ROTATE if self.rotate else 0) | (_lib.EDIT_SCALE if self.scale else 0)
        t.D1[:] = D[1:4, 1:4].reshape(-1).tolist()
        t.D2[:] = D[4:9, 4:9].reshape(-1).tolist()
        t.D3[:] = D[9:16, 9:16].reshape(-1).tolist()
        return t


# ---- validation -------------------------------------------------------------------------------------------------------------
def _check_tensor(t, what, fn, shape=None):
    """type, dtype and shape: everything that can be wrong before the device matters"""
    if not torch.is_tensor(t):
        raise ValueError(f"{fn}: {what} must be a tensor")
    if t.dtype != torch.float32:
        raise ValueError(f"{fn}: {what} must be torch.float32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{fn}: {what} has shape {tuple(t.shape)}, expected {tuple(shape)}")


def _check_selection(selection, P, dev, fn):
    if selection is None:
        return
    if not torch.is_tensor(selection) or selection.dtype not in (torch.bool, torch.uint8) or tuple(selection.shape) != (P,):
        raise ValueError(f"{fn}: selection must be a bool or uint8 tensor of shape ({P},)")
    if selection.device != dev:
        raise ValueError(f"{fn}: selection is on {selection.device}, expected {dev}")


def _check_device(tensors, dev, fn):
    """every tensor on the model's device, that device a GPU, every tensor contiguous"""
    for what, t in tensors:
        if t.device != dev:
            raise ValueError(f"{fn}: {what} is on {t.device}, expected {dev}")
    if dev.type != "cuda":
        raise RuntimeError(_NO_CPU)
    for what, t in tensors:
        if not t.is_contiguous():
            raise ValueError(f"{fn}: {what} must be contiguous")


def _pivot(pivot, fn):
    """("device", tensor) | ("derived", name) | ("host", float64 [3])"""
    if isinstance(pivot, str):
        if pivot not in _PIVOTS:
            raise ValueError(f"{fn}: pivot must be one of {_PIVOTS}, three numbers or a device tensor [3], got {pivot!r}")
        return ("host", np.zeros(3)) if pivot == "origin" else ("derived", pivot)
    if torch.is_tensor(pivot) and pivot.device.type != "cpu":
        _check_tensor(pivot, "pivot", fn, (3,))
        return "device", pivot
    a = _host_array(pivot, "pivot", fn)
    if a.shape != (3,):
        raise ValueError(f"{fn}: pivot must be three numbers, got shape {a.shape}")
    return "host", a


def _bounds_launch(xyz, selection, invert, dev):
    """count int32 [1] and out float32 [12] = lo | hi | centroid | center"""
    lib = _lib.load()
    P = int(xyz.shape[0])
    nbytes = int(lib.goi_edit_bounds_workspace_bytes(P))
    if nbytes == 0:
        raise ValueError(f"selection_bounds: P = {P} is out of range (P < 2^31)")
    ws = workspace(nbytes, dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    out = torch.empty(12, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.goi_edit_bounds(P, ptr(xyz), ptr(selection), 1 if invert else 0, ptr(count), ptr(out), ptr(ws), stream(dev)),
              ValueError)
    return count, out


def selection_bounds(xyz, selection=None, invert=False):
    """{"count": int32 [1], "lo", "hi", "centroid", "center": float32 [3]} of the selected rows of xyz [P, 3], all on the
    device, without a read-back.  lo / hi are exact; the centroid is a float64 sum in a fixed order (no float atomics: the same
    bits on every run) divided by the count and rounded once; center = 0.5 lo + 0.5 hi.  An empty selection gives count 0,
    lo = +inf, hi = -inf, centroid = center = 0."""
    fn = "selection_bounds"
    _check_tensor(xyz, "xyz", fn)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{fn}: xyz has shape {tuple(xyz.shape)}, expected [P, 3]")
    dev = xyz.device
    _check_selection(selection, int(xyz.shape[0]), dev, fn)
    _check_device([("xyz", xyz)], dev, fn)
    sel = None if selection is None else selection.contiguous()
    count, out = _bounds_launch(xyz.detach(), sel, invert, dev)
    return {"count": count, "lo": out[0:3], "hi": out[3:6], "centroid": out[6:9], "center": out[9:12]}


# ---- the edit ---------------------------------------------------------------------------------------------------------------
def transform(g, selection=None, *, rotation=None, translation=None, scale=1.0, pivot="centroid", invert=False, moments=True):
    """x' = p + t + s R (x - p) on the selected Gaussians of `g`, in place (see the module docstring).

    selection: bool / uint8 [P] on the model's device (non-zero selects), None = every row; invert=True edits the rows whose
    byte is 0 instead, as render(..., mask_invert=) does.  rotation: a proper 3x3 rotation matrix or a (w, x, y, z) quaternion;
    translation: three numbers; scale: s > 0; pivot: "centroid" (of the selection), "center" (of its bounding box), "origin",
    three host numbers or a device tensor [3].  Host values may be sequences, numpy arrays or CPU tensors.  One kernel launch,
    plus the two of selection_bounds for a derived pivot; no host synchronisation."""
    fn = "transform"
    sim = Similarity(rotation, translation, scale, fn)
    kind, pv = _pivot(pivot, fn)
    if getattr(g, "_semantics_masks", None) is not None:
        raise ValueError(f"{fn}: the model has a semantic mask set (set_semantic_masks); clear it (set_semantic_masks(None)) "
                         "before editing the model")
    xyz = g._xyz
    _check_tensor(xyz, "_xyz", fn)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{fn}: _xyz has shape {tuple(xyz.shape)}, expected [P, 3]")
    P, dev = int(xyz.shape[0]), xyz.device
    params = {"_xyz": xyz}
    for attr in ("_rotation", "_scaling"):
        _check_tensor(getattr(g, attr), attr, fn, (P,) + _ROW[attr])
        params[attr] = getattr(g, attr)
    rest = g._features_rest
    _check_tensor(rest, "_features_rest", fn)
    if rest.dim() != 3 or rest.shape[0] != P or rest.shape[2] != 3 or int(rest.shape[1]) + 1 not in (1, 4, 9, 16):
        raise ValueError(f"{fn}: _features_rest has shape {tuple(rest.shape)}, expected [{P}, M - 1, 3] with M in (1, 4, 9, 16)")
    params["_features_rest"] = rest
    M = int(rest.shape[1]) + 1
    _check_selection(selection, P, dev, fn)
    tensors = list(params.items())
    if kind == "device":
        tensors.append(("pivot", pv))
    # the first moments a rotation turns
    mom = {}
    if moments and sim.rotate:
        opt, groups = densify._groups(g, fn)
        for name, attr in (("xyz", "_xyz"), ("rotation", "_rotation"), ("f_rest", "_features_rest")):
            if opt is None or name not in groups:
                continue
            st = opt.state.get(params[attr], None)
            if not st or "exp_avg" not in st:
                continue
            m = st["exp_avg"]
            _check_tensor(m, f"the exp_avg of group {name!r}", fn, tuple(params[attr].shape))
            mom[attr] = m
            tensors.append((f"the exp_avg of group {name!r}", m))
    _check_device(tensors, dev, fn)
    sel = None if selection is None else selection.contiguous()

    lib = _lib.load()
    general = sim.rotate or sim.scale  # a pure translation involves no pivot
    pivot_dev = None
    host_pivot = np.zeros(3)
    if general and kind == "derived":
        _count, out = _bounds_launch(xyz.detach(), sel, invert, dev)
        pivot_dev = out[6:9] if pv == "centroid" else out[9:12]
    elif general and kind == "device":
        pivot_dev = pv.detach()
    elif kind == "host":
        host_pivot = pv
    t = sim.struct(host_pivot)
    m_rest = mom.get("_features_rest") if M > 1 else None
    with torch.cuda.device(dev):
        check(lib.goi_edit_transform(P, M, ptr(sel), 1 if invert else 0, ctypes.byref(t), ptr(xyz), ptr(params["_rotation"]),
                                     ptr(params["_scaling"]), ptr(rest), ptr(mom.get("_xyz")), ptr(mom.get("_rotation")),
                                     ptr(m_rest), ptr(pivot_dev), stream(dev)), ValueError)
    # the kernel wrote through raw pointers: tell everything that watches version counters (the geometry cache)
    written = [xyz]
    if sim.rotate:
        written += [params["_rotation"]] + ([rest] if M > 1 else [])
        written += [m for attr, m in mom.items() if attr != "_features_rest" or M > 1]
    if sim.scale:
        written.append(params["_scaling"])
    for w in written:
        torch.autograd.graph.increment_version(w)


def move(g, selection, direction):
    """gui/main_edit.py:1512-1548 (obj_move): _xyz[selection] += direction, bit for bit, without the boolean index's host
    synchronisation.  The Adam state is untouched (a translation moves no moment)."""
    transform(g, selection, translation=direction, pivot="origin")


def transform_camera(camera, *, rotation=None, translation=None, scale=1.0, pivot="origin"):
    """The scene.Camera that sees the transformed model as `camera` saw the original one: its centre goes through the same
    similarity and its axes turn with R.  For row-vector world_view_transform = W2C^T with W2C = [Rc | tc] the new W2C is
    [Rc R^T | Rc (s p - R^T (p + t)) + s tc]; full_proj_transform and camera_center are rebuilt.  Under s != 1 every view-space
    coordinate is multiplied by s: the picture is the same and the depth map s times the old one.  pivot: "origin" or three
    numbers (a device tensor is read back).  Formed in float64, stored as fp32."""
    from .scene import ZFAR, ZNEAR, Camera, projection_matrix
    fn = "transform_camera"
    sim = Similarity(rotation, translation, scale, fn)
    if isinstance(pivot, str):
        if pivot != "origin":
            raise ValueError(f"{fn}: pivot must be \"origin\" or three numbers (a camera has no selection to derive one from)")
        p = np.zeros(3)
    else:
        p = _host_array(pivot, "pivot", fn)
        if p.shape != (3,):
            raise ValueError(f"{fn}: pivot must be three numbers, got shape {p.shape}")
    w2c = np.asarray(camera.world_view_transform, dtype=np.float64).T
    Rc, tc = w2c[:3, :3], w2c[:3, 3]
    new = np.eye(4)
    new[:3, :3] = Rc @ sim.R.T
    new[:3, 3] = Rc @ (sim.s * p - sim.R.T @ (p + sim.t)) + sim.s * tc
    view_T = np.ascontiguousarray(new.T).astype(np.float32)
    proj_T = np.ascontiguousarray(projection_matrix(ZNEAR, ZFAR, camera.FoVx, camera.FoVy).T)
    full = (view_T @ proj_T.astype(np.float32)).astype(np.float32)
    center = np.linalg.inv(view_T.astype(np.float64))[3, :3].astype(np.float32)
    return Camera(camera.image_width, camera.image_height, camera.FoVx, camera.FoVy, view_T, full, center)
