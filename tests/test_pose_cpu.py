"""goi_hyperplane_amd.pose without a GPU: the SH rotation generators, the mathematics of the pose gradient against central
differences of the full transform in float64 (tests/pose_reference.py), the camera's sign, twist_rotation, the C surface and every
refusal the entry and the module make before they need a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import edit, pose
from goi_hyperplane_amd.scene import make_camera
from tests import densify_reference as dref
from tests import pose_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
MIS = C.c_void_p((1 << 20) + 4)
N = None
GEN = (C.c_float * 48)()
PIV = (C.c_float * 3)()


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


# ---- generators -------------------------------------------------------------------------------------------------------------
def _expm(A):
    """exp(A) by scaling and squaring of a Taylor series: |A / 2^s| <= 2^-4, 18 terms (the remainder is below 1e-30)"""
    s = max(0, int(np.ceil(np.log2(max(np.abs(A).sum(axis=1).max(), 1e-300)))) + 4)
    B = A / 2.0 ** s
    E, term = np.eye(len(A)), np.eye(len(A))
    for k in range(1, 19):
        term = term @ B / k
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_generators_are_skew_close_under_the_bracket_and_exponentiate_to_sh_rotation(degree):
    G = pose.sh_generators(degree)
    n = (degree + 1) ** 2
    assert G.shape == (3, n, n) and G.dtype == np.float64
    assert not G[:, 0, :].any() and not G[:, :, 0].any()  # band 0 is a constant: it does not turn
    assert np.abs(G + G.transpose(0, 2, 1)).max() <= 1e-12
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        assert np.abs(G[a] @ G[b] - G[b] @ G[a] - G[c]).max() <= 1e-12, (a, b, c)
    theta = 0.7
    for k in range(3):
        omega = np.zeros(3)
        omega[k] = theta
        err = np.abs(_expm(theta * G[k]) - edit.sh_rotation(pose.twist_rotation(omega), degree)).max()
        print(f"degree {degree} axis {k}: |exp(theta G) - D| = {err:.2e}")
        assert err <= 1e-11, (k, err)
    if degree:
        assert np.abs(G).max() > 0.9


def test_generators_are_formed_once_and_have_the_compiled_pattern():
    G = pose.sh_generators(3)
    assert tuple(int(np.count_nonzero(G[k])) for k in range(3)) == pose.NONZEROS == (18, 18, 12)
    G[0, 1, 2] = 99.0  # a copy: the cached generators are not the caller's to change
    assert pose.sh_generators(3)[0, 1, 2] != 99.0
    for M, want in ((1, (0, 0, 0)), (4, (2, 2, 2)), (9, (8, 8, 6)), (16, (18, 18, 12))):
        got = tuple(len(pose.generator_entries(k, M)) for k in range(3))
        assert got == want, M
        for k in range(3):  # a narrower model's entries are a prefix: the kernel takes the first n of the 48 values' groups
            assert pose.generator_entries(k, M) == pose.generator_entries(k, 16)[:got[k]]
    # the tables csrc/pose.hip compiles in are these entries, in this order
    src = open(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "pose.hip")).read()
    tables = re.findall(r"constexpr Entry e\[(\d+)\] = \{(.*?)\};", src, flags=re.S)
    assert [int(n) for n, _ in tables] == [18, 18, 12]
    for k, (_, body) in enumerate(tables):
        pairs = [(int(i), int(j)) for i, j in re.findall(r"\{(\d+), (\d+)\}", body)]
        assert pairs == pose.generator_entries(k, 16), k
    packed = np.array(pose._packed_generators()[:], dtype=np.float32)
    want = np.concatenate([[G32 for G32 in (pose.sh_generators(3)[k][i + 1, j + 1] for i, j in pose.generator_entries(k))]
                           for k in range(3)]).astype(np.float32)
    assert np.array_equal(packed, want)
    with pytest.raises(ValueError):
        pose.sh_generators(4)


# ---- the mathematics --------------------------------------------------------------------------------------------------------
def _problem(P, M, seed):
    rng = np.random.default_rng(seed)
    shapes = {"_xyz": (P, 3), "_rotation": (P, 4), "_scaling": (P, 3), "_features_rest": (P, M - 1, 3)}
    arrays = {k: rng.normal(size=s) for k, s in shapes.items()}
    a = {k: rng.normal(size=s) for k, s in shapes.items()}
    return arrays, a, rng.random(P) < 0.6, rng.normal(size=3)


def _loss(a, arrays):
    return float(sum((a[k] * np.sin(arrays[k])).sum() for k in ref.KEYS))


@pytest.mark.parametrize("M,invert", [(16, False), (4, False), (16, True)])
def test_the_gradient_is_the_derivative_of_the_transform(M, invert):
    """L = sum a sin(theta) over all four tensors; exact_sums of the float64 pieces against central differences of
    L(apply(+-h e_k)) at h = 1e-5: truncation h^2 plus round-off 1e-16 / h is about 1e-10 of the largest component"""
    arrays, a, sel, pivot = _problem(37, M, seed=M + invert)
    eff = ref.effective(sel, invert, 37)
    grads = {k: a[k] * np.cos(arrays[k]) for k in ref.KEYS}
    got, _ = ref.exact_sums(ref.terms(arrays, grads, eff, pivot, dtype=np.float64))
    h = 1e-5
    want = np.zeros(7)
    for k in range(7):
        e = np.zeros(7)
        e[k] = h
        want[k] = (_loss(a, ref.apply(e, arrays, eff, pivot)) - _loss(a, ref.apply(-e, arrays, eff, pivot))) / (2 * h)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"M {M} invert {invert}: relative error {rel:.2e}")
    assert rel <= 1e-7, (got, want)
    assert np.abs(want).min() > 1e-3 * np.abs(want).max()  # every component is exercised


def test_apply_is_the_identity_at_zero_and_matches_edit_reference():
    arrays, _a, sel, pivot = _problem(37, 16, seed=3)
    out = ref.apply(np.zeros(7), arrays, sel, pivot)
    for k in ref.KEYS:
        assert np.abs(out[k] - arrays[k]).max() <= 1e-13, k  # (sh_rotation is the identity to a few 1e-15, by sampling)
    tau = np.array([0.2, -0.1, 0.3, 0.5, 0.25, -1.0, 0.1])
    from tests import edit_reference as eref
    c = eref.constants(pose.twist_rotation(tau[:3]), tau[3:6], np.exp(tau[6]), pivot, dtype=np.float64)
    want = eref.transform(arrays, sel, c)
    out = ref.apply(tau, arrays, sel, pivot)
    for k in ref.KEYS:
        assert np.abs(out[k] - want[k]).max() <= 1e-13, k


def _w2c(cam_w2c, R, t, p):
    """edit.transform_camera's documented formula at s = 1, float64: [Rc R^T | Rc (p - R^T (p + t)) + tc]"""
    Rc, tc = cam_w2c[:3, :3], cam_w2c[:3, 3]
    return Rc @ R.T, Rc @ (p - R.T @ (p + t)) + tc


def test_the_camera_gradient_is_minus_the_whole_model_gradient():
    """L = sum a sin(W2C x): minus the whole-model gradient about p against central differences of moving the camera by
    T(+-h e_k) about p, the six components"""
    rng = np.random.default_rng(5)
    P = 37
    x, a, p = rng.normal(size=(P, 3)), rng.normal(size=(P, 3)), rng.normal(size=3)
    cam = make_camera(96, 64, yaw=0.3, pitch=-0.2).world_view_transform.astype(np.float64).T

    def loss(tau):
        Rv, tv = _w2c(cam, pose.twist_rotation(tau[:3]), tau[3:6], p)
        return float((a * np.sin(x @ Rv.T + tv)).sum())

    Rc, tc = cam[:3, :3], cam[:3, 3]
    g_x = (a * np.cos(x @ Rc.T + tc)) @ Rc
    arrays = {"_xyz": x, "_rotation": np.zeros((P, 4)), "_scaling": np.zeros((P, 3)), "_features_rest": np.zeros((P, 15, 3))}
    grads = {"_xyz": g_x, "_rotation": None, "_scaling": None, "_features_rest": None}
    model, _ = ref.exact_sums(ref.terms(arrays, grads, np.ones(P, bool), p, dtype=np.float64))
    h = 1e-5
    want = np.zeros(6)
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        want[k] = (loss(e) - loss(-e)) / (2 * h)
    rel = np.abs(-model[:6] - want).max() / np.abs(want).max()
    print(f"camera: relative error {rel:.2e}")
    assert rel <= 1e-7, (model, want)
    # and the restated formula is what transform_camera builds
    tau = np.array([0.1, -0.2, 0.15, 0.3, -0.2, 0.1])
    moved = edit.transform_camera(make_camera(96, 64, yaw=0.3, pitch=-0.2), rotation=pose.twist_rotation(tau[:3]),
                                  translation=tau[3:], pivot=p).world_view_transform.astype(np.float64).T
    Rv, tv = _w2c(cam, pose.twist_rotation(tau[:3]), tau[3:], p)
    assert np.abs(moved[:3, :3] - Rv).max() <= 1e-6 and np.abs(moved[:3, 3] - tv).max() <= 1e-5


# ---- twist_rotation ---------------------------------------------------------------------------------------------------------
def test_twist_rotation():
    assert np.array_equal(pose.twist_rotation((0.0, 0.0, 0.0)), np.eye(3))
    rng = np.random.default_rng(1)
    for scale in (1e-12, 1e-6, 1e-3, 0.05, 1.0, 3.0):
        omega = scale * rng.normal(size=3)
        R = pose.twist_rotation(omega)
        assert R.dtype == np.float64 and R.shape == (3, 3)
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-15, scale
        assert np.abs(R - edit._quat_to_matrix(ref.twist_quaternion(omega))).max() <= 1e-15, scale
        assert np.abs(R @ omega - omega).max() <= 4e-15 * max(1.0, scale)  # the axis stays
    assert np.allclose(pose.twist_rotation((0, 0, np.pi / 2)), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    for bad in ((1.0, 2.0), "x", (0.0, float("nan"), 0.0)):
        with pytest.raises(ValueError):
            pose.twist_rotation(bad)


# ---- the C surface ----------------------------------------------------------------------------------------------------------
def test_header_and_symbol_table_agree(lib):
    from goi_hyperplane_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    declared = set(re.findall(r"^(?:int|size_t) (goi_pose_\w+)\(", hdr, flags=re.M))
    assert declared == set(_lib.POSE_SYMBOLS) == {"goi_pose_gradient_workspace_bytes", "goi_pose_gradient"}
    assert _lib.POSE_SYMBOLS in _lib.LATER_TABLES and _lib.POSE_SYMBOLS not in _lib.SYMBOL_TABLES
    assert not set(_lib.POSE_SYMBOLS) & set(_lib.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name)
        assert name in hdr.split("#define GOI_RASTER_ABI_VERSION")[0], f"{name} is not in the list of later additions"
    assert lib.goi_raster_abi_version() == _lib.ABI_VERSION == 9
    size = lib.goi_pose_gradient_workspace_bytes
    assert size(-1) == 0 and size(1 << 31) == 0
    assert 0 < size(0) <= size(1) <= size(1000) <= size(10 ** 6) == size((1 << 31) - 1) < (1 << 20)  # the partials are bounded


def test_the_package_exports_the_module():
    import goi_hyperplane_amd
    assert goi_hyperplane_amd.pose is pose and "pose" in goi_hyperplane_amd.__all__
    with pytest.raises(AttributeError):
        goi_hyperplane_amd.no_such_module


#            P  M  sel inv xyz rot rest g_x g_r g_l g_c gen  piv  pdev count out ws stream
REFUSED = [
    ((-1, 16, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: need 0 <= P < 2^31"),
    ((1 << 31, 16, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: need 0 <= P < 2^31"),
    ((8, 0, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: M must be 1, 4, 9 or 16"),
    ((8, 5, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: M must be 1, 4, 9 or 16"),
    ((8, 16, N, 0, F, F, F, N, N, N, N, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: every gradient pointer is NULL"),
    ((8, 16, N, 0, N, F, F, F, F, F, F, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: a gradient is given whose parameter pointer is NULL"),
    ((8, 16, N, 0, F, N, F, F, F, F, F, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: a gradient is given whose parameter pointer is NULL"),
    ((8, 16, N, 0, F, F, N, F, F, F, F, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: a gradient is given whose parameter pointer is NULL"),
    ((8, 1, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, F, F, F, N), "goi_pose_gradient: M = 1 has no features_rest gradient"),
    ((8, 16, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, F, N, F, N), "goi_pose_gradient: a required pointer is NULL"),
    ((8, 16, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, N, F, F, N), "goi_pose_gradient: a required pointer is NULL"),
    ((8, 16, N, 0, F, F, F, F, F, F, F, N, PIV, N, F, F, F, N), "goi_pose_gradient: a required pointer is NULL"),
    ((8, 16, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, F, F, N, N), "goi_pose_gradient: NULL workspace"),
    ((8, 16, N, 0, F, F, F, F, F, F, F, GEN, PIV, N, F, F, MIS, N), "goi_pose_gradient: workspace must be 256-byte aligned"),
    ((0, 16, N, 0, N, N, N, N, N, N, N, GEN, PIV, N, N, N, F, N), "goi_pose_gradient: a required pointer is NULL"),
]


@pytest.mark.parametrize("args,message", REFUSED)
def test_entry_refusals_before_any_device_call(lib, args, message):
    assert lib.goi_pose_gradient(*args) == -1
    assert lib.goi_raster_last_error().decode() == message


# ---- the module's own refusals ----------------------------------------------------------------------------------------------
def _cpu_model(P=8, M=16, grads=True):
    g = dref.make_model(P, torch.device("cpu"), optimizer=None, M=M)
    if grads:
        for attr in pose.GRADS:
            getattr(g, attr).grad = torch.ones_like(getattr(g, attr))
    return g


def test_every_bad_argument_is_refused_without_a_gpu():
    P = 8
    g = _cpu_model(P)
    for kw in (dict(pivot="middle"), dict(pivot=(1.0, 2.0)), dict(pivot=(0.0, 0.0, float("nan")))):
        with pytest.raises(ValueError, match="pivot"):
            pose.gradient(g, None, **kw)
    for sel in (torch.zeros(P, dtype=torch.float32), torch.zeros(P + 1, dtype=torch.bool), [True] * P):
        with pytest.raises(ValueError, match="selection"):
            pose.gradient(g, sel)
    with pytest.raises(ValueError, match="selection is on"):
        pose.gradient(g, torch.zeros(P, dtype=torch.bool, device="meta"))
    with pytest.raises(ValueError, match="run a backward first"):
        pose.gradient(_cpu_model(P, grads=False))
    with pytest.raises(ValueError, match="run a backward first"):
        pose.camera_gradient(_cpu_model(P, grads=False))
    with pytest.raises(ValueError, match="run a backward first"):
        pose.gradient(g, grads=dict.fromkeys(pose.GRADS))
    for bad in ({"_xyz": torch.ones(P, 3)}, [torch.ones(P, 3)] * 4, dict.fromkeys(pose.GRADS + ("_opacity",))):
        with pytest.raises(ValueError, match="grads must be a dict"):
            pose.gradient(g, grads=bad)
    for attr, t in (("_xyz", torch.ones(P, 4)), ("_rotation", torch.ones(P, 4, dtype=torch.float64)),
                    ("_scaling", torch.ones(P + 1, 3)), ("_features_rest", torch.ones(P, 45)), ("_xyz", np.ones((P, 3), np.float32))):
        grads = {k: torch.ones_like(getattr(g, k)) for k in pose.GRADS}
        grads[attr] = t
        with pytest.raises(ValueError, match=f"the gradient of {attr}"):
            pose.gradient(g, grads=grads)
    for attr, t in (("_xyz", torch.zeros(P, 4)), ("_rotation", torch.zeros(P, 3)), ("_scaling", torch.zeros(P, 3, dtype=torch.float16)),
                    ("_features_rest", torch.zeros(P, 14, 3))):
        bad = _cpu_model(P)
        setattr(bad, attr, t)
        with pytest.raises(ValueError, match=attr):
            pose.gradient(bad)


def test_cpu_tensors_are_refused_loudly_and_a_semantic_mask_is_not():
    g = _cpu_model()
    g.set_semantic_masks(torch.ones(8))  # nothing is written: the mask is no reason to refuse
    sel = torch.zeros(8, dtype=torch.bool)
    for call in (lambda: pose.gradient(g, sel), lambda: pose.gradient(g, None, pivot="origin"),
                 lambda: pose.gradient(g, sel, pivot=(0.1, 0.2, 0.3), invert=True), lambda: pose.camera_gradient(g),
                 lambda: pose.camera_gradient(g, pivot=(0.0, 0.0, -5.0)),
                 lambda: pose.gradient(g, grads={"_xyz": torch.ones(8, 3), "_rotation": None, "_scaling": None, "_features_rest": None})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        pose.fit(g, sel, lambda: None, iterations=1, lr_rotation=-1.0, lr_translation=0.1)
    R, t, s, history = pose.fit(g, sel, lambda: None, iterations=0, lr_rotation=0.01, lr_translation=0.1)
    assert np.array_equal(R, np.eye(3)) and not t.any() and s == 1.0 and history == {"loss": [], "steps": []}
