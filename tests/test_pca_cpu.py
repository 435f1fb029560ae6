"""The PCA stage without a GPU: the numpy restatement (tests/pca_reference.py) against sklearn's own results
(tests/golden/ref_pca_pins.npz, made by tests/golden/make_pca_golden.py), the C ABI's declarations and exports, and the
argument checks of goi_hyperplane_amd.pca, which all run on the host before anything is launched."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

from tests import pca_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "golden", "ref_pca_pins.npz")
HEADER = os.path.join(HERE, "..", "include", "goi_raster.h")
FUNCTIONS = ("goi_semantic_pca_workspace_bytes", "goi_semantic_pca_accumulate", "goi_semantic_pca_solve",
             "goi_semantic_pca_apply")


@pytest.fixture(scope="module")
def pins():
    with np.load(PINS) as z:
        return {k: z[k] for k in z.files}


def cases(pins):
    return sorted(k[:-2] for k in pins if k.endswith("_x"))


def test_the_pinned_cases_are_well_conditioned(pins):
    """A ratio of at least 1.3 between the top four eigenvalues: a near-degenerate basis is not a defect of anyone's code."""
    assert cases(pins) == ["s10", "s16", "s16_offset", "s17", "s3", "s32"]
    for name in cases(pins):
        w = ref.eigenvalues(pins[name + "_x"])[:4]
        assert (w[:-1] / w[1:]).min() >= 1.3, (name, w)


def test_restatement_reproduces_sklearn(pins):
    for name in cases(pins):
        x = pins[name + "_x"]
        assert x.dtype == np.float32
        b = ref.fit(x)
        scale = np.abs(x).max()
        assert b.count == len(x)
        assert np.abs(b.mean - pins[name + "_mean"]).max() <= 1e-9 * scale, name
        assert np.array_equal(np.sign(b.components), np.sign(pins[name + "_components"])), name
        assert np.abs(b.components - pins[name + "_components"]).max() <= 1e-9, name
        assert np.abs(b.explained_variance - pins[name + "_explained_variance"]).max() <= 1e-9 * b.explained_variance[0], name
        assert np.abs(ref.project(x, b) - pins[name + "_transform"]).max() <= 1e-9 * scale, name
        for k in range(3):  # the sign rule itself
            assert b.components[k, np.argmax(np.abs(b.components[k]))] > 0


def test_restatement_mask_and_small_counts():
    x = ref.sample(10, 200, 7)
    m = np.random.default_rng(1).uniform(size=200) < 0.4
    a, b = ref.fit(x, m), ref.fit(x[m])
    assert a.count == m.sum() and np.array_equal(a.components, b.components) and np.array_equal(a.mean, b.mean)
    one = ref.fit(x[:1])
    assert one.count == 1 and not one.components.any() and not one.explained_variance.any() and np.array_equal(one.mean, x[0])
    none = ref.fit(x, np.zeros(200, bool))
    assert none.count == 0 and not none.components.any() and not none.mean.any()


def test_normalisations_are_float32_and_handle_the_edges():
    q = np.array([[0.0, 1.0, -1.0], [np.nan, 4.0, 2.0], [8.0, -8.0, 0.5]], np.float32)
    ev = np.array([4.0, 1.0, 0.0], np.float32)
    s = ref.sigma(q, ev, 2.0)
    assert s.dtype == np.float32
    assert s[0, 0] == 0.5 and s[1, 0] == 0.0 and s[2, 0] == 1.0  # q = 0; a NaN; 8 / (4 * 2) = 1 -> 1.5 clamped
    assert s[0, 1] == 0.75 and s[2, 1] == 0.0
    assert s[0, 2] == 0.0 and s[1, 2] == 1.0  # sigma = 0: the denominator is 4 * FLT_MIN
    assert ref.sigma(np.zeros((2, 3), np.float32), np.zeros(3, np.float32))[0, 0] == 0.5
    m = ref.minmax(q)
    assert m.dtype == np.float32 and m[0, 0] == 0.0 and m[2, 0] == 1.0 and np.isnan(m[1, 0])
    assert m[2, 1] == 0.0 and m[1, 1] == 1.0
    assert not ref.minmax(np.full((5, 3), 3.25, np.float32)).any()  # range 0 gives 0


def test_header_declares_and_library_exports_the_functions():
    hdr = open(HEADER).read()
    for fn in FUNCTIONS:
        assert re.search(rf"^(size_t|int) {fn}\(", hdr, re.M), fn
    val = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))  # noqa: E731
    from goi_hyperplane_amd import _lib, pca
    assert (val("GOI_PCA_PLANAR"), val("GOI_PCA_ROWS")) == (pca.PLANAR, pca.ROWS)
    assert (val("GOI_PCA_RAW"), val("GOI_PCA_SIGMA"), val("GOI_PCA_MINMAX")) == (pca.RAW, pca.SIGMA, pca.MINMAX)
    assert (val("GOI_PCA_MIN_DIM"), val("GOI_PCA_MAX_DIM")) == (pca.MIN_DIM, pca.MAX_DIM) == (3, 32)
    assert "#define GOI_PCA_BASIS_FLOATS(S) (4 * (S) + 5)" in hdr and pca.basis_floats(16) == 69
    lib = _lib.load()
    for fn in FUNCTIONS:
        assert fn in _lib.SYMBOLS and hasattr(lib, fn), fn
    assert lib.goi_semantic_pca_workspace_bytes(16, 0) > 0 and lib.goi_semantic_pca_workspace_bytes(0, 3) == 72
    assert lib.goi_semantic_pca_workspace_bytes(2, 0) == 0 and lib.goi_semantic_pca_workspace_bytes(33, 0) == 0
    assert lib.goi_semantic_pca_workspace_bytes(32, 0) > lib.goi_semantic_pca_workspace_bytes(16, 0)


def test_c_abi_refuses_bad_arguments():
    """The checks come before anything touches a device."""
    import ctypes as C
    from goi_hyperplane_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 1024)()
    p = C.cast(buf, C.c_void_p)
    assert lib.goi_semantic_pca_accumulate(p, 0, 2, 10, None, 1, p, None) < 0 and b"S" in lib.goi_raster_last_error()
    assert lib.goi_semantic_pca_accumulate(p, 0, 33, 10, None, 1, p, None) < 0
    assert lib.goi_semantic_pca_accumulate(p, 0, 16, 0, None, 1, p, None) < 0
    assert lib.goi_semantic_pca_accumulate(p, 0, 16, 2 ** 31, None, 1, p, None) < 0
    assert lib.goi_semantic_pca_accumulate(p, 2, 16, 10, None, 1, p, None) < 0
    assert lib.goi_semantic_pca_accumulate(None, 0, 16, 10, None, 1, p, None) < 0
    assert lib.goi_semantic_pca_solve(16, None, p, None) < 0 and lib.goi_semantic_pca_solve(40, p, p, None) < 0
    assert lib.goi_semantic_pca_apply(p, 0, 16, 10, 1, p, 3, 2.0, p, 0, None, None) < 0
    assert lib.goi_semantic_pca_apply(p, 0, 16, 10, 1, p, 2, 2.0, p, 0, None, None) < 0  # MINMAX without a workspace
    assert lib.goi_semantic_pca_apply(p, 0, 16, 10, 1, p, 1, 0.0, p, 0, None, None) < 0  # k_sigma = 0
    assert lib.goi_semantic_pca_apply(p, 0, 16, 10, 70000, p, 0, 2.0, p, 0, None, None) < 0
    assert lib.goi_semantic_pca_apply(p, 0, 16, 10, 0, p, 0, 2.0, p, 0, None, None) == 0  # no views: nothing to do


def test_cpu_tensors_raise():
    from goi_hyperplane_amd import pca
    x = torch.zeros(16, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pca.fit(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pca.fit(torch.zeros(50, 16), layout="rows")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pca.fit_views([x, x])
    basis = pca.PcaBasis(torch.zeros(pca.basis_floats(16)), 16)
    assert basis.components.shape == (3, 16) and basis.mean.shape == (16,) and basis.explained_variance.shape == (3,)
    for normalize in ("raw", "sigma", "minmax"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pca.transform(x, basis, normalize=normalize)

    class Pc:
        get_semantics = torch.zeros(100, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pca.fit_gaussians(Pc())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pca.gaussian_colors(Pc())


def test_bad_arguments_raise_before_any_launch():
    from goi_hyperplane_amd import pca
    with pytest.raises(ValueError, match="3 <= S <= 32"):
        pca.fit(torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match="3 <= S <= 32"):
        pca.fit(torch.zeros(33, 8, 8))
    with pytest.raises(ValueError, match="3 <= S <= 32"):
        pca.fit(torch.zeros(100, 40), layout="rows")
    with pytest.raises(ValueError, match="mask has 63 elements"):
        pca.fit(torch.zeros(16, 8, 8), mask=torch.zeros(63, dtype=torch.bool))
    with pytest.raises(TypeError, match="mask"):
        pca.fit(torch.zeros(16, 8, 8), mask=torch.zeros(64))
    with pytest.raises(ValueError, match="unknown layout"):
        pca.fit(torch.zeros(16, 8, 8), layout="columns")
    with pytest.raises(TypeError, match="float32"):
        pca.fit(torch.zeros(16, 8, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="no maps"):
        pca.fit_views([])
    with pytest.raises(ValueError, match="channel count"):
        pca.fit_views([torch.zeros(16, 4, 4), torch.zeros(10, 4, 4)])
    with pytest.raises(ValueError, match="2 maps but 1 masks"):
        pca.fit_views([torch.zeros(16, 4, 4), torch.zeros(16, 4, 4)], masks=[None])
    basis = pca.PcaBasis(torch.zeros(pca.basis_floats(16)), 16)
    x = torch.zeros(16, 8, 8)
    with pytest.raises(ValueError, match="unknown normalize"):
        pca.transform(x, basis, normalize="zscore")
    with pytest.raises(ValueError, match="unknown layout"):
        pca.transform(x, basis, layout="columns")
    with pytest.raises(ValueError, match="the basis has 16 channels"):
        pca.transform(torch.zeros(10, 8, 8), basis)
    with pytest.raises(ValueError, match="k_sigma"):
        pca.transform(x, basis, normalize="sigma", k_sigma=0.0)
    with pytest.raises(ValueError, match="out must be"):
        pca.transform(x, basis, out=torch.zeros(3, 8, 9))
    with pytest.raises(TypeError, match="PcaBasis"):
        pca.transform(x, torch.zeros(69))
    with pytest.raises(ValueError, match="PcaBasis"):
        pca.PcaBasis(torch.zeros(68), 16)


def test_semantics_is_a_frame_mode():
    from goi_hyperplane_amd import semantic
    assert semantic.FRAME_MODES == ("image", "depth", "alpha", "semantics")
