"""The hyperplane fit kernels (csrc/osh.hip: osh_fit_k<REG>, osh_counts_k) directly: short fits at every shape class the
kernel accepts, on every path that accepts them, against the float64 per-code fit of tests/osh_reference.py.

A fit of 1 to 64 epochs keeps an fp32 evaluation within a few 1e-7 of float64, so the gates are not the fixed 1e-3 of
tests/test_gpu_osh.py but, per case and quantity x, 8 d32_x + 8 eps32 scale_x with d32_x the error of the case's own fp32
restatement (osh_reference.direct_tolerances).  tests/test_osh_cpu.py holds every case's margins at least 32 margin errors
away from the decision points {-1, 0, 1}, so the IoU trace is demanded exactly.  MAX_RATIO collects the largest
|x_gpu - x_f64| / tolerance per quantity (docs/MEASUREMENT_LOG.md records them)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests.osh_reference import (DIRECT_CASES, GUARD_FACTOR, KINK_B0, KINK_SHAPES, counts_of, direct_case, direct_tolerances,
                                 kink_case, kink_of, make_direct_inputs, margin_error, reference_fits)

pytestmark = pytest.mark.gpu
LR = 0.01
MAX_RATIO = {}  # quantity -> (largest error / tolerance seen, where)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    for q, (r, what) in sorted(MAX_RATIO.items()):
        print(f"\nosh direct: largest error / tolerance of {q}: {r:.3f} ({what})", end="")


def _paths(n_codes, D):
    return (0, 1) if D == 256 and n_codes <= 320 else (1,)


def _fit(dev, path, lut, counts, HW, w0, b0, max_epochs, target_iou=2.0):
    """fit_hyperplanes_counts on host arrays: lut [n, D], counts [K, 2, n], w0 [K, D], b0 [K]."""
    from goi_hyperplane_amd import _lib
    from goi_hyperplane_amd.semantic import fit_hyperplanes_counts
    _lib.set_option("osh_path", path)
    try:
        return fit_hyperplanes_counts(torch.tensor(lut, device=dev), torch.tensor(np.asarray(counts), dtype=torch.int32, device=dev),
                                      HW, torch.tensor(w0, device=dev), torch.tensor(b0, dtype=torch.float32, device=dev), lr=LR,
                                      max_epochs=max_epochs, target_iou=target_iou, return_trace=True)
    finally:
        _lib.set_option("osh_path", 0)


def _fit_case(dev, path, case):
    w, b, fits = _fit(dev, path, case["lut"], case["counts"][None], case["HW"], case["w0"][None], [case["b0"]], case["epochs"])
    return w[0].cpu().numpy().astype(np.float64), float(b[0].double()), fits[0]


@functools.lru_cache(maxsize=None)
def _direct_reference(name):
    case = direct_case(name)
    r64, r32 = reference_fits(case, LR)
    return case, r64, direct_tolerances(r64, r32, LR)


@functools.lru_cache(maxsize=None)
def _kink_reference(shape, b0):
    case = kink_case(shape, b0)
    r64, r32 = reference_fits(case, LR)
    return case, r64, direct_tolerances(r64, r32, LR)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _assert_fit(w, b, fit, r64, tol, what):
    """Epochs, init IoU and IoU trace exactly; loss trace, w, b and OSHFit.loss within the case's bound."""
    assert fit.epochs == r64["epochs"], (what, fit.epochs)
    t = fit.trace.numpy()
    assert t.shape == r64["trace"].shape, what
    assert _same(fit.init_iou, r64["init_iou"]), (what, fit.init_iou, r64["init_iou"])
    assert _same(t[:, 1], r64["trace"][:, 1]), (what, t[:, 1], r64["trace"][:, 1])
    assert _same(fit.iou, r64["iou"]), what
    errs = dict(trace=np.abs(t[:, 0] - r64["trace"][:, 0]).max(), loss=abs(fit.loss - r64["loss"]),
                w=np.abs(w - r64["w"]).max(), b=abs(b - r64["b"]))
    for q, e in errs.items():
        print(f"{what}: {q} error {e:.3g} tolerance {tol[q]:.3g}")
        if tol[q] > 0 and e / tol[q] > MAX_RATIO.get(q, (-1.0, ""))[0]:
            MAX_RATIO[q] = (float(e / tol[q]), what)
    for q, e in errs.items():
        assert e <= tol[q], (what, q, float(e), tol[q])


# ---- a. every case against float64, on every path that accepts it ---------------------------------------------------------
@pytest.mark.parametrize("name,path", [(n, p) for n, c in DIRECT_CASES.items() for p in _paths(c["n_codes"], c["D"])])
def test_direct_case_matches_float64(dev, name, path):
    case, r64, tol = _direct_reference(name)
    w, b, fit = _fit_case(dev, path, case)
    _assert_fit(w, b, fit, r64, tol, f"{name} path {path}")


# ---- b. exact kinks, one epoch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b0", KINK_B0)
@pytest.mark.parametrize("shape,path", [(s, p) for s in KINK_SHAPES for p in _paths(DIRECT_CASES[s]["n_codes"], DIRECT_CASES[s]["D"])])
def test_decisions_at_the_kink(dev, shape, path, b0):
    """w0 = 0: every margin of the first pass is b0 exactly.  b0 = 1: every present code is predicted, positives add no
    loss but pass their gradient (1 - o = 0 >= 0); b0 = -1: the mirror for negatives, nothing predicted; b0 = 0: nothing
    predicted (o > 0 is false), both hinges active."""
    case, r64, tol = _kink_reference(shape, b0)
    w, b, fit = _fit_case(dev, path, case)
    what = f"kink {shape} b0 {b0} path {path}"
    P, N = case["counts"].astype(np.float64)
    assert fit.init_iou == (P.sum() / (P.sum() + N.sum()) if b0 > 0 else 0.0), what
    want_loss = {1.0: 2 * N.sum(), -1.0: 2 * P.sum(), 0.0: P.sum() + N.sum()}[b0] / case["HW"]
    assert fit.trace[0, 0].item() == pytest.approx(want_loss, rel=1e-6), what
    assert fit.trace[0, 0].item() == pytest.approx(r64["trace"][0, 0], rel=1e-6), what
    _assert_fit(w, b, fit, r64, tol, what)


def test_kink_without_positives_has_a_nan_init_iou(dev):
    """b0 = -1 and b0 = 0 with no positive pixel: nothing is predicted and the union is empty."""
    case = kink_case("17x65_e1", -1.0)
    case["counts"] = np.stack([np.zeros_like(case["counts"][0]), case["counts"].sum(0)])
    for b0 in (-1.0, 0.0):
        case["b0"] = b0
        r64, r32 = reference_fits(case, LR)
        assert np.isnan(r64["init_iou"]) and kink_of(r64["margins"][1:]) >= GUARD_FACTOR * margin_error(r64, r32, first=1)
        w, b, fit = _fit_case(dev, 1, case)
        assert np.isnan(fit.init_iou)
        _assert_fit(w, b, fit, r64, direct_tolerances(r64, r32, LR), f"no positives, b0 {b0}")


# ---- c. nothing present -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,path", [("17x65_e1", 1), ("40x256_e1", 0), ("40x256_e1", 1)])
@pytest.mark.parametrize("HW", (1, 4096))
def test_nothing_present(dev, shape, path, HW):
    case = direct_case(shape)
    zero = np.zeros_like(case["counts"])
    w, b, fits = _fit(dev, path, case["lut"], zero[None], HW, case["w0"][None], [case["b0"]], max_epochs=8)
    fit = fits[0]
    assert fit.epochs == 1 and np.isnan(fit.iou) and np.isnan(fit.init_iou) and fit.loss == 0.0
    assert fit.trace.shape == (1, 2) and fit.trace[0, 0].item() == 0.0 and np.isnan(fit.trace[0, 1].item())
    assert torch.equal(w[0].cpu(), torch.tensor(case["w0"])) and torch.equal(b.cpu(), torch.tensor([case["b0"]], dtype=torch.float32))


# ---- d. the two paths agree bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", (1.0, 0.4))
@pytest.mark.parametrize("n_codes", (1, 15, 16, 17, 319, 320))
def test_paths_agree_bit_for_bit(dev, n_codes, frac):
    lut, counts, w0 = make_direct_inputs(7, n_codes, 256, 4096, frac)
    runs = {}
    for path in (0, 1):
        for rerun in (0, 1):
            w, b, fits = _fit(dev, path, lut, counts[None], 4096, w0[None], [0.1], max_epochs=64)
            assert fits[0].epochs == 64
            runs[path, rerun] = (w, b, fits[0].trace)
    for key in ((0, 1), (1, 0), (1, 1)):
        for x, y in zip(runs[0, 0], runs[key]):
            assert torch.equal(x, y), (n_codes, frac, key)


# ---- e. batches on the generic path -----------------------------------------------------------------------------------------
def test_generic_batch_equals_single_fits(dev):
    """One launch of five fits over one 321 x 100 LUT -- dense, sparse, all-positive, all-zero and single-code counts, each
    with its own w0 and b0 -- equals the five single fits bit for bit."""
    n, D, HW = 321, 100, 4096
    lut, dense, _ = make_direct_inputs(11, n, D, HW, 1.0)
    sparse = make_direct_inputs(12, n, D, HW, 0.1)[1]
    allpos = np.stack([dense.sum(0), np.zeros(n, np.int64)])
    zero = np.zeros((2, n), np.int64)
    single = zero.copy()
    single[:, 200] = (HW - 1000, 1000)
    counts = np.stack([dense, sparse, allpos, zero, single])
    assert (sparse.sum(0) > 0).sum() < 64
    rng = np.random.default_rng(13)
    w0 = (rng.normal(size=(5, D)) * 0.1).astype(np.float32)
    b0 = [0.1, -0.2, 0.3, 0.86, -0.05]
    wk, bk, fk = _fit(dev, 1, lut, counts, HW, w0, b0, max_epochs=64)
    assert [f.epochs for f in fk] == [64, 64, 64, 1, 64]
    for i in range(5):
        ws, bs, fs = _fit(dev, 1, lut, counts[i:i + 1], HW, w0[i:i + 1], b0[i:i + 1], max_epochs=64)
        assert torch.equal(ws[0], wk[i]) and torch.equal(bs[0], bk[i]), i
        assert fs[0].epochs == fk[i].epochs and torch.equal(fs[0].trace.view(torch.int64), fk[i].trace.view(torch.int64)), i  # (bits: NaN IoU)
        assert _same([fs[0].loss, fs[0].iou, fs[0].init_iou], [fk[i].loss, fk[i].iou, fk[i].init_iou]), i
    assert len({tuple(w.tolist()) for w in wk.cpu()}) == 5


# ---- f. osh_counts_k's promises ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", (1, 255, 256, 257, 2049))
@pytest.mark.parametrize("n_codes", (1, 1000))
def test_counts_skip_foreign_codes_and_take_any_nonzero_byte(dev, n_codes, HW):
    from goi_hyperplane_amd.semantic import osh_counts
    rng = np.random.default_rng(1000 * n_codes + HW)
    foreign = np.array([-1, n_codes, 2 ** 31 - 1, -2 ** 31], np.int64)
    idx = np.where(rng.random(HW) < 0.25, foreign[rng.integers(0, 4, HW)], rng.integers(0, n_codes, HW)).astype(np.int32)
    if HW >= 4:
        idx[np.linspace(0, HW - 1, 4).astype(int)] = foreign  # each foreign value at least once, first and last pixel included
    pos = np.array([0, 1, 2, 255], np.uint8)[rng.integers(0, 4, HW)]
    valid = (idx >= 0) & (idx < n_codes)
    want = counts_of(idx[valid], pos[valid], n_codes)
    assert want.sum() == valid.sum() and (HW < 255 or (0 < valid.sum() < HW))
    got = osh_counts(torch.tensor(idx, device=dev), torch.tensor(pos, device=dev), n_codes)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)


# ---- g. the wrapper's limits ------------------------------------------------------------------------------------------------
def test_wrapper_limits(dev):
    from goi_hyperplane_amd.semantic import fit_hyperplanes_counts

    def call(n=30, D=64, HW=15, K=1, counts_shape=None, w_shape=None, b_shape=None, **kw):
        return fit_hyperplanes_counts(torch.rand(n, D, device=dev),
                                      torch.ones(counts_shape or (K, 2, n), dtype=torch.int32, device=dev), HW,
                                      torch.zeros(w_shape or (K, D), device=dev), torch.zeros(b_shape or (K,), device=dev), **kw)

    for bad in (dict(n=1001), dict(D=1025), dict(HW=0), dict(HW=2 ** 31), dict(max_epochs=0), dict(counts_shape=(1, 2, 29)),
                dict(counts_shape=(2, 2, 30)), dict(counts_shape=(1, 30, 2)), dict(w_shape=(1, 63)), dict(w_shape=(2, 64)),
                dict(b_shape=(2,)), dict(b_shape=(1, 1))):
        with pytest.raises(ValueError):
            call(**bad)
    call(n=1000, D=1024, HW=2 ** 31 - 1, max_epochs=1)  # the limits themselves are accepted
    w, b, fits = call(K=0, return_trace=True)
    assert w.shape == (0, 64) and b.shape == (0,) and fits == []
    torch.cuda.synchronize()
