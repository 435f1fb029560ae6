"""goi_hyperplane_amd.edit without a GPU: the SH rotation matrices against tests/sh_basis_ref.py in float64, the float32
restatement of the edit (tests/edit_reference.py) against its float64 twin within running-error bounds, the camera's similarity,
the C surface, and every refusal the module makes before it needs a device."""
import os
import re
import types

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import edit
from goi_hyperplane_amd.scene import make_camera
from tests import densify_reference as dref
from tests import edit_reference as ref
from tests.sh_basis_ref import sh_basis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(6)


def _dirs(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


# ---- sh_rotation ------------------------------------------------------------------------------------------------------------
def test_sh_rotation_of_the_identity_is_the_identity():
    for degree in range(4):
        D = edit.sh_rotation(np.eye(3), degree)
        assert D.dtype == np.float64 and D.shape == ((degree + 1) ** 2,) * 2
        assert np.abs(D - np.eye((degree + 1) ** 2)).max() <= 1e-12
    assert np.abs(edit.sh_rotation([1.0, 0.0, 0.0, 0.0]) - np.eye(16)).max() <= 1e-12  # the identity quaternion


@pytest.mark.parametrize("seed", SEEDS)
def test_sh_rotation_is_block_diagonal_and_orthogonal(seed):
    D = edit.sh_rotation(ref.random_rotation(seed))
    blocks = np.zeros((16, 16), dtype=bool)
    for l in range(4):
        blocks[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = True
    assert not D[~blocks].any()
    assert abs(D[0, 0] - 1.0) <= 1e-12
    assert np.abs(D @ D.T - np.eye(16)).max() <= 1e-12
    assert np.array_equal(edit.sh_rotation(ref.random_rotation(seed), 2), D[:9, :9])  # a lower degree is the leading block


@pytest.mark.parametrize("seed", SEEDS)
def test_sh_rotation_is_multiplicative_in_this_order(seed):
    R1, R2 = ref.random_rotation(seed), ref.random_rotation(100 + seed)
    D12 = edit.sh_rotation(R1 @ R2)
    assert np.abs(D12 - edit.sh_rotation(R1) @ edit.sh_rotation(R2)).max() <= 1e-12
    assert np.abs(D12 - edit.sh_rotation(R2) @ edit.sh_rotation(R1)).max() > 1e-3  # and not in the other


@pytest.mark.parametrize("seed", SEEDS)
def test_rotated_coefficients_reproduce_the_function_in_the_rotated_frame(seed):
    """sum_k c'_k Y_k(R d) = sum_k c_k Y_k(d) with the basis of tests/sh_basis_ref.py, float64"""
    R = ref.random_rotation(seed)
    D = edit.sh_rotation(R)
    d = _dirs(200, 50 + seed)
    c = np.random.default_rng(70 + seed).normal(size=16)
    Y = sh_basis(torch.tensor(d), 3, 16).numpy()
    Yr = sh_basis(torch.tensor(d @ R.T), 3, 16).numpy()  # rows (R d)^T
    assert Y.dtype == np.float64
    assert np.abs(Yr @ (D @ c) - Y @ c).max() <= 1e-12


def test_a_quaternion_and_its_matrix_give_the_same_rotation():
    for seed in SEEDS:
        q = np.random.default_rng(seed).normal(size=4)
        R = edit._quat_to_matrix(q / np.linalg.norm(q))
        assert np.abs(edit._rotation_matrix(q, "t") - R).max() <= 1e-15  # any non-zero quaternion is normalised
        back = edit._matrix_to_quat(R)
        assert np.abs(edit._quat_to_matrix(back) - R).max() <= 1e-14 and back[0] >= 0
    # the branches of the matrix -> quaternion conversion a half turn takes (trace -1)
    for axis in range(3):
        R = -np.eye(3)
        R[axis, axis] = 1.0
        assert np.abs(edit._quat_to_matrix(edit._matrix_to_quat(R)) - R).max() <= 1e-15


# ---- the float32 restatement ------------------------------------------------------------------------------------------------
def _arrays(P, M, seed, dtype):
    g = np.random.default_rng(seed)
    a = {"_xyz": g.normal(size=(P, 3)) * 2, "_rotation": g.normal(size=(P, 4)), "_scaling": g.normal(size=(P, 3)) - 3,
         "_features_rest": 0.3 * g.normal(size=(P, M - 1, 3)), "m_xyz": 1e-3 * g.normal(size=(P, 3)),
         "m_rotation": 1e-3 * g.normal(size=(P, 4)), "m_features_rest": 1e-3 * g.normal(size=(P, M - 1, 3))}
    return {k: v.astype(np.float32).astype(dtype) for k, v in a.items()}  # the same fp32 values in either precision


@pytest.mark.parametrize("M", [1, 4, 9, 16])
@pytest.mark.parametrize("scale", [1.0, 1.7])
def test_float32_restatement_is_within_the_running_error_bound_of_float64(M, scale):
    P = 300
    sel = np.random.default_rng(3).random(P) < 0.5
    kw = dict(rotation=ref.random_rotation(M), translation=(0.3, -0.2, 0.1), scale=scale, pivot=(0.1, 0.2, -0.1))
    c32, c64 = ref.constants(dtype=np.float32, **kw), ref.constants(dtype=np.float64, **kw)
    a32, a64 = _arrays(P, M, 5, np.float32), _arrays(P, M, 5, np.float64)
    o32, o64 = ref.transform(a32, sel, c32), ref.transform(a64, sel, c64)
    for k in o32:
        assert o32[k].dtype == np.float32 and o64[k].dtype == np.float64
        assert np.array_equal(o32[k][~sel], a32[k][~sel]), k
    err = lambda k: np.abs(o32[k][sel].astype(np.float64) - o64[k][sel])  # noqa: E731
    assert (err("_xyz") <= ref.position_bound(c64, a64["_xyz"][sel])).all()
    assert (err("_rotation") <= ref.quat_bound(c64, a64["_rotation"][sel])).all()
    assert (err("m_rotation") <= ref.quat_bound(c64, a64["m_rotation"][sel])).all()
    assert (err("_features_rest") <= ref.rest_bound(c64, a64["_features_rest"][sel])).all()
    assert (err("m_features_rest") <= ref.rest_bound(c64, a64["m_features_rest"][sel])).all()
    lin = dict(c64, p=np.zeros(3), t=np.zeros(3), s=1.0)  # a moment gets R m only
    assert (err("m_xyz") <= ref.position_bound(lin, a64["m_xyz"][sel])).all()
    assert np.abs(o64["m_xyz"][sel] - a64["m_xyz"][sel] @ c64["R"].T).max() <= 1e-15
    if scale == 1.0:
        assert np.array_equal(o32["_scaling"], a32["_scaling"])
    else:
        assert (err("_scaling") <= ref.gamma(2) * (np.abs(a64["_scaling"][sel]) + abs(c64["log_s"]))).all()
    # the quaternion keeps its norm, the activated covariance is R Sigma R^T
    n0, n1 = np.linalg.norm(a64["_rotation"][sel], axis=1), np.linalg.norm(o64["_rotation"][sel], axis=1)
    assert np.abs(n1 / n0 - 1).max() <= 1e-14
    Rq = lambda q: dref.rotation_matrices(torch.tensor(q)).numpy()  # noqa: E731
    assert np.abs(Rq(o64["_rotation"][sel]) - c64["R"][None] @ Rq(a64["_rotation"][sel])).max() <= 1e-13


def test_pure_translation_is_the_single_add():
    P = 200
    sel = np.random.default_rng(1).random(P) < 0.5
    a = _arrays(P, 16, 2, np.float32)
    t = np.array([0.1, -0.25, 0.033], dtype=np.float32)
    for pivot in ((0.0, 0.0, 0.0), (5.0, -3.0, 2.0)):  # no pivot is involved
        out = ref.transform(a, sel, ref.constants(translation=t, pivot=pivot))
        want = a["_xyz"].copy()
        want[sel] += t
        assert np.array_equal(out["_xyz"], want)
        for k in a:
            assert k == "_xyz" or np.array_equal(out[k], a[k]), k


# ---- the camera -------------------------------------------------------------------------------------------------------------
def _inverse(R, t, s, p):
    """x = p + t' + s' R' (x' - p) undoes x' = p + t + s R (x - p)"""
    return dict(rotation=R.T, translation=-(R.T @ np.asarray(t)) / s, scale=1.0 / s, pivot=p)


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_transform_camera_and_its_inverse_return_the_camera(scale):
    cam = make_camera(96, 64, yaw=0.3, pitch=-0.2)
    R, t, p = ref.random_rotation(4), (0.3, -0.2, 0.1), (0.1, 0.2, -0.1)
    moved = edit.transform_camera(cam, rotation=R, translation=t, scale=scale, pivot=p)
    assert np.abs(moved.world_view_transform - cam.world_view_transform).max() > 1e-2
    back = edit.transform_camera(moved, **_inverse(R, t, scale, p))
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert getattr(back, k).dtype == np.float32
        assert np.abs(getattr(back, k) - getattr(cam, k)).max() <= 1e-6, k
    assert (back.image_width, back.image_height, back.FoVx, back.FoVy) == (cam.image_width, cam.image_height, cam.FoVx, cam.FoVy)
    # the moved camera sees the moved points where the camera saw the points (view space: times s)
    x = np.random.default_rng(0).normal(size=(50, 3))
    x2 = np.asarray(p) + np.asarray(t) + scale * (x - np.asarray(p)) @ R.T
    view = lambda c, v: np.c_[v, np.ones(len(v))] @ c.world_view_transform.astype(np.float64)  # noqa: E731
    assert np.abs(view(moved, x2)[:, :3] - scale * view(cam, x)[:, :3]).max() <= 1e-5
    # at s = 1 the new W2C is [Rc R^T | Rc (p - R^T (p + t)) + tc]
    if scale == 1.0:
        w2c = cam.world_view_transform.astype(np.float64).T
        Rc, tc = w2c[:3, :3], w2c[:3, 3]
        new = moved.world_view_transform.astype(np.float64).T
        assert np.abs(new[:3, :3] - Rc @ R.T).max() <= 1e-6
        assert np.abs(new[:3, 3] - (Rc @ (np.asarray(p) - R.T @ (np.asarray(p) + np.asarray(t))) + tc)).max() <= 1e-6
        assert np.abs(moved.camera_center - (np.asarray(p) + np.asarray(t) + R @ (cam.camera_center - np.asarray(p)))).max() <= 1e-5


# ---- which scene can carry the picture's invariance gate --------------------------------------------------------------------
def _oracle_motion(seed, rot_seed, scale):
    """max |difference| per map between the CPU oracle's frame of a scene and its frame of the numpy-restated edit of that scene
    seen by transform_camera's camera (depth divided by the scale), and the oracle's `fragile` map of the untouched frame"""
    import copy
    from goi_hyperplane_amd.scene import make_scene
    from oracle import oracle
    sc = make_scene(3000, S=4, seed=seed, log_scale_mean=-2.5)
    cam = make_camera(96, 64, yaw=0.3, pitch=-0.2)
    f0 = oracle.from_scene(sc, cam).forward()
    kw = dict(rotation=ref.random_rotation(rot_seed), translation=(0.3, -0.2, 0.1), scale=scale, pivot=(0.1, 0.2, -0.1))
    out = ref.transform({"_xyz": sc.means3D, "_rotation": sc.rotations, "_scaling": np.log(sc.scales),
                         "_features_rest": sc.shs[:, 1:].copy()}, np.ones(sc.P, bool), ref.constants(**kw))
    sc2 = copy.copy(sc)
    sc2.means3D, sc2.scales = out["_xyz"], np.exp(out["_scaling"]).astype(np.float32)
    sc2.rotations = (out["_rotation"] / np.linalg.norm(out["_rotation"], axis=1, keepdims=True)).astype(np.float32)
    sc2.shs = np.concatenate([sc.shs[:, :1], out["_features_rest"]], axis=1)
    f1 = oracle.from_scene(sc2, edit.transform_camera(cam, **kw)).forward()
    diff = {"render": np.abs(f1.color - f0.color).max(axis=0), "semantics": np.abs(f1.semantic - f0.semantic).max(axis=0),
            "depth": np.abs(f1.depth / scale - f0.depth).max(axis=0), "alpha": np.abs(f1.alpha - f0.alpha).max(axis=0)}
    return diff, f0.fragile.reshape(64, 96) != 0


def test_the_oracle_s_own_response_to_a_rigid_motion_picks_the_scale_case():
    """The reference's own error decides which scene tests/test_gpu_edit.py uses for its s = 2 invariance case (gate 1e-4, no
    pixel excluded).  No code under test runs here: the CPU oracle renders a scene, and the numpy restatement's edit of it seen
    from the moved camera.  Scene 1 stays an order of magnitude inside the gate on every motion tried (at most 1.1e-5 over
    rotations 40 .. 47 at s = 1 and 2; the test runs the case the GPU test uses and one more).  Scene 0 does not: at rotation
    40, s = 1, ONE pixel -- row 3, column 39, which the oracle marks `fragile` in the untouched frame -- moves by 2.0e-3 in
    colour, while every pixel that is not fragile stays inside the gate.  So the case the issue leaves open goes to scene 1."""
    gate = 1e-4
    for rot_seed, scale in ((41, 2.0), (40, 2.0)):
        diff, _ = _oracle_motion(1, rot_seed, scale)
        for k, d in diff.items():
            assert d.max() < gate, (rot_seed, scale, k, float(d.max()))
    diff, fragile = _oracle_motion(0, 40, 1.0)
    assert fragile[3, 39] and 10 <= fragile.sum() <= 40
    over = np.zeros((64, 96), dtype=bool)
    for k, d in diff.items():
        over |= d >= gate
    assert not (over & ~fragile).any()  # whatever leaves the gate on scene 0 is a pixel the oracle itself calls fragile


# ---- the C surface ----------------------------------------------------------------------------------------------------------
def test_header_and_symbol_table_agree():
    from goi_hyperplane_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    declared = set(re.findall(r"^(?:int|size_t) (goi_edit_\w+)\(", hdr, flags=re.M))
    assert declared == set(_lib.EDIT_SYMBOLS) and len(declared) == 3
    assert _lib.EDIT_SYMBOLS in _lib.SYMBOL_TABLES
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
        assert name in hdr[:hdr.index("#define GOI_RASTER_ABI_VERSION")]  # listed under ABI 8's later additions
    assert int(re.search(r"#define GOI_EDIT_ROTATE (\d+)", hdr).group(1)) == _lib.EDIT_ROTATE
    assert int(re.search(r"#define GOI_EDIT_SCALE (\d+)", hdr).group(1)) == _lib.EDIT_SCALE
    assert lib.goi_edit_bounds_workspace_bytes(1000) > 0 and lib.goi_edit_bounds_workspace_bytes(1 << 31) == 0
    assert lib.goi_edit_bounds_workspace_bytes(10 ** 9) < (1 << 20)  # the partials are bounded


def test_transform_struct_layout_matches_c(tmp_path):
    import ctypes
    import subprocess
    from goi_hyperplane_amd._lib import GoiEditTransform
    fields = [f[0] for f in GoiEditTransform._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goi_raster.h"\nint main(void){\n'
                   + "".join(f'printf("{f} %zu\\n", offsetof(GoiEditTransform, {f}));\n' for f in fields)
                   + 'printf("sizeof %zu\\n", sizeof(GoiEditTransform));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for f in fields:
        assert getattr(GoiEditTransform, f).offset == int(out[f]), f
    assert ctypes.sizeof(GoiEditTransform) == int(out["sizeof"])


def test_the_struct_holds_the_constants_rounded_once():
    R = ref.random_rotation(2)
    sim = edit.Similarity(R, (0.5, 0.25, -1.0), 1.5)
    t = sim.struct((0.1, 0.2, 0.3))
    c = ref.constants(R, (0.5, 0.25, -1.0), 1.5, (0.1, 0.2, 0.3))
    assert np.array_equal(np.array(t.R[:], np.float32).reshape(3, 3), c["R"])
    assert np.array_equal(np.array(t.q[:], np.float32), c["q"]) and np.array_equal(np.array(t.t[:], np.float32), c["t"])
    assert np.array_equal(np.array(t.pivot[:], np.float32), c["p"])
    assert np.float32(t.s) == c["s"] and np.float32(t.log_s) == c["log_s"] and t.flags == 3
    for got, want in zip((t.D1, t.D2, t.D3), c["D"]):
        assert np.array_equal(np.array(got[:], np.float32).reshape(want.shape), want)
    assert edit.Similarity(None, (1, 2, 3), 1.0).struct((0, 0, 0)).flags == 0
    assert edit.Similarity(None, None, 2.0).struct((0, 0, 0)).flags == 2
    assert edit.Similarity(np.eye(3), None, 1.0).struct((0, 0, 0)).flags == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _cpu_model(P=8, M=16):
    return dref.make_model(P, torch.device("cpu"), optimizer=None, M=M)


def test_every_bad_argument_is_refused_without_a_gpu():
    g = _cpu_model()
    P = 8
    half = np.sqrt(0.5)
    bad = [
        dict(rotation=np.eye(3) * 1.001),                                          # not orthonormal
        dict(rotation=np.eye(3) + 3e-6),                                           # |R^T R - I| > 1e-6
        dict(rotation=np.diag([1.0, 1.0, -1.0])),                                  # a mirror
        dict(rotation=-np.eye(3)),                                                 # a point reflection: det -1 as well
        dict(rotation=np.eye(4)), dict(rotation=[1.0, 0.0, 0.0]), dict(rotation=[0.0, 0.0, 0.0, 0.0]),
        dict(rotation=[[float("nan")] * 3] * 3), dict(rotation="x"),
        dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale="big"),
        dict(translation=(1.0, 2.0)), dict(translation=(1.0, 2.0, float("inf"))),
        dict(pivot="middle"), dict(pivot=(1.0, 2.0)), dict(pivot=(0.0, 0.0, float("nan"))),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            edit.transform(g, None, **kw)
    for sel in (torch.zeros(P, dtype=torch.float32), torch.zeros(P + 1, dtype=torch.bool), torch.zeros((P, 1), dtype=torch.bool),
                [True] * P):
        with pytest.raises(ValueError, match="selection"):
            edit.transform(g, sel, translation=(1, 0, 0))
    with pytest.raises(ValueError, match="selection is on"):  # a selection on another device than the model
        edit.transform(g, torch.zeros(P, dtype=torch.bool, device="meta"), translation=(1, 0, 0))
    with pytest.raises(ValueError, match="selection is on"):
        edit.selection_bounds(g._xyz.detach(), torch.zeros(P, dtype=torch.bool, device="meta"))
    # a fine float32 rotation matrix and a quaternion pass the argument checks and reach the device check
    for rot in (ref.random_rotation(0).astype(np.float32), torch.tensor([half, 0.0, half, 0.0]), [[1, 0, 0], [0, 0, -1], [0, 1, 0]]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            edit.transform(g, None, rotation=rot)


def test_wrong_model_tensors_are_refused_without_a_gpu():
    P = 8
    for attr, t in (("_xyz", torch.zeros(P, 4)), ("_xyz", torch.zeros(P, 3, dtype=torch.float64)), ("_rotation", torch.zeros(P, 3)),
                    ("_rotation", torch.zeros(P + 1, 4)), ("_scaling", torch.zeros(P, 3, dtype=torch.float16)),
                    ("_scaling", torch.zeros(P, 1)), ("_features_rest", torch.zeros(P, 14, 3)),
                    ("_features_rest", torch.zeros(P, 15, 4)), ("_features_rest", torch.zeros(P, 45)),
                    ("_features_rest", torch.zeros(P, 15, 3, dtype=torch.float64)), ("_rotation", np.zeros((P, 4), np.float32))):
        g = _cpu_model(P)
        setattr(g, attr, t)
        with pytest.raises(ValueError, match=attr):
            edit.transform(g, None, rotation=np.eye(3))
    g = _cpu_model(P)
    g.set_semantic_masks(torch.ones(P))
    with pytest.raises(ValueError, match="semantic mask"):
        edit.transform(g, None, translation=(1, 0, 0))
    with pytest.raises(ValueError, match="semantic mask"):
        edit.move(g, None, (1, 0, 0))
    with pytest.raises(ValueError):
        edit.selection_bounds(torch.zeros(P, 4))
    with pytest.raises(ValueError):
        edit.selection_bounds(torch.zeros(P, 3, dtype=torch.float64))
    with pytest.raises(ValueError):  # an optimizer group the model does not know, as densify refuses it
        g = _cpu_model(P)
        g.optimizer = types.SimpleNamespace(param_groups=[{"name": "colour", "params": [g._xyz]}], state={})
        edit.transform(g, None, rotation=np.eye(3))


def test_cpu_tensors_are_refused_loudly():
    g = _cpu_model()
    sel = torch.zeros(8, dtype=torch.bool)
    for call in (lambda: edit.transform(g, sel, translation=(1, 0, 0)), lambda: edit.transform(g, None, scale=2.0, pivot="center"),
                 lambda: edit.move(g, sel, (0.1, 0, 0)), lambda: edit.selection_bounds(g._xyz.detach(), sel),
                 lambda: edit.transform(g, None, rotation=np.eye(3), pivot=torch.zeros(3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        edit.transform_camera(make_camera(32, 32), pivot="centroid")
    with pytest.raises(ValueError):
        edit.transform_camera(make_camera(32, 32), rotation=np.diag([1.0, -1.0, 1.0]))
    with pytest.raises(ValueError):
        edit.sh_rotation(np.eye(3), degree=4)
