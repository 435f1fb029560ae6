"""The hyperplane fine-tune without a GPU: the restated LinearSVM (step / eval_forward / hinge_loss / calculate_iou of
networks.py:12-67 and utils/image_utils.py:59-70) replays the reference's own loop pinned in
tests/golden/ref_osh_pins.npz, the float64 per-code form (tests/osh_reference.py) agrees with it, the OSH entry
points reject bad input, and every direct case of tests/test_gpu_osh_direct.py is far from every decision boundary."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests.osh_reference import (DIRECT_CASES, GUARD_FACTOR, KINK_B0, KINK_SHAPES, counts_of, direct_case, direct_tolerances,
                                 fit_per_code, iou_flips, kink_case, kink_of, margin_error, reference_fits)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ("a", "b", "c", "d")


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLD, "ref_osh_pins.npz"))


# intra-op threads of the run that made the pins.  The blocking of torch's CPU GEMMs and reductions follows the thread
# count, and over thousands of SGD epochs a different blocking drifts past 1e-6 (and can move the stopping epoch), so
# the replay runs at this count whatever the host's CPU count is.
PIN_THREADS = 8


@pytest.fixture
def pin_threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(PIN_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(prev)


@pytest.mark.parametrize("name", CASES)
def test_restated_linear_svm_replays_reference(pins, name, pin_threads):
    """Same statements, same CPU fp32 arithmetic: epochs, init IoU and IoU trace exactly; the loss trace and the final
    w / b to 1e-6 relative (at the pins' thread count the replay is bit-exact on the machine that made them; another
    CPU's kernels may round differently)."""
    from goi_hyperplane_amd.semantic import LinearSVM
    lut = torch.tensor(pins[f"{name}_lut"])
    idx = torch.tensor(pins[f"{name}_idx"]).long()
    gt = torch.tensor(pins[f"{name}_gt"]).float().reshape(-1, 1)
    svm = LinearSVM(set_bias=float(pins[f"{name}_set_bias"]), input_dim=lut.shape[1])
    svm.weight_set(torch.tensor(pins[f"{name}_w0"]).reshape(1, -1))
    assert float(svm.linear.bias.detach()) == float(pins[f"{name}_b0"])
    sem_feature = lut[idx]
    normed = sem_feature / sem_feature.norm(dim=-1, keepdim=True)
    init_iou = svm.eval_forward(normed, gt)
    np.testing.assert_array_equal(np.asarray(init_iou), pins[f"{name}_init_iou"])
    trace, epoch, iou = [], 0, 0
    while epoch < 8000 and iou < 0.9:
        loss, iou = svm.step(normed, gt)
        trace.append((loss.item(), iou))
        epoch += 1
    trace = np.array(trace)
    ref = pins[f"{name}_trace"]
    assert epoch == int(pins[f"{name}_epochs"])
    np.testing.assert_array_equal(trace[:, 1], ref[:, 1])
    np.testing.assert_allclose(trace[:, 0], ref[:, 0], rtol=1e-6, atol=0)
    np.testing.assert_allclose(svm.linear.weight.detach().numpy().reshape(-1), pins[f"{name}_w"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(float(svm.linear.bias.detach()), float(pins[f"{name}_b"]), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("name", CASES)
def test_per_code_float64_matches_reference(pins, name):
    lut = pins[f"{name}_lut"]
    res = fit_per_code(lut, counts_of(pins[f"{name}_idx"], pins[f"{name}_gt"], lut.shape[0]), int(np.prod(pins[f"{name}_hw"])),
                       pins[f"{name}_w0"], float(pins[f"{name}_b0"]))
    epochs = int(pins[f"{name}_epochs"])
    assert res["epochs"] == epochs
    assert iou_flips(res["trace"][:, 1], pins[f"{name}_trace"][:, 1]) <= max(2, epochs // 200)
    np.testing.assert_array_equal(np.asarray(res["init_iou"]), pins[f"{name}_init_iou"])
    w_ref = pins[f"{name}_w"]
    assert np.abs(res["w"] - w_ref).max() <= 1e-3 * np.abs(w_ref).max()
    if name == "c":
        assert epochs == 1 and np.isnan(pins["c_trace"][0, 1])
    if name == "a":
        assert epochs < 8000 and pins["a_trace"][-1, 1] >= 0.9
    if name == "b":
        assert epochs == 8000


def test_hinge_loss_and_iou_helpers():
    from goi_hyperplane_amd.semantic import calculate_iou, hinge_loss
    o = torch.tensor([2.0, 0.5, -0.5, -2.0, 1.0])
    y = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0])
    assert hinge_loss(o, y).item() == pytest.approx((0 + 0.5 + 0.5 + 0 + 2.0) / 5)
    assert calculate_iou(y > 0, o > 0) == 2 / 3
    assert np.isnan(calculate_iou(torch.zeros(3, dtype=torch.bool), torch.zeros(3, dtype=torch.bool)))
    # clamp(min=0)'s gradient passes at the kink (1 - o * label == 0)
    from goi_hyperplane_amd.semantic import LinearSVM
    svm = LinearSVM(input_dim=2)
    assert "optimizer" not in svm.state_dict() and set(svm.state_dict()) == {"linear.weight", "linear.bias"}
    assert svm.optimizer.param_groups[0]["lr"] == 0.01
    o = torch.tensor([1.0], requires_grad=True)
    hinge_loss(o, torch.tensor([1.0])).backward()
    assert o.grad.item() == -1.0


def test_osh_entry_points_reject_bad_input():
    from goi_hyperplane_amd.semantic import (LinearSVM, SemanticModel, fit_hyperplane, fit_hyperplanes_counts,
                                             osh_counts)
    mlp = SemanticModel(dim_in=4, dim_out=1001, num_layer=1, use_bias=True, device="cpu")
    sem = torch.zeros(4, 3, 5)
    with pytest.raises(ValueError):  # more codes than the reference's [:, :1000] slice keeps
        fit_hyperplane(sem, mlp, torch.rand(1001, 256), torch.zeros(15), LinearSVM())
    mlp = SemanticModel(dim_in=4, dim_out=30, num_layer=1, use_bias=True, device="cpu")
    with pytest.raises(ValueError):  # mask size
        fit_hyperplane(sem, mlp, torch.rand(30, 256), torch.zeros(16), LinearSVM())
    with pytest.raises(ValueError):  # LUT / LinearSVM feature size
        fit_hyperplane(sem, mlp, torch.rand(30, 128), torch.zeros(15), LinearSVM())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_hyperplane(sem, mlp, torch.rand(30, 256), torch.zeros(15), LinearSVM())
    with pytest.raises(ValueError):
        osh_counts(torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.bool), 1001)
    with pytest.raises(ValueError):
        osh_counts(torch.zeros(5, dtype=torch.int32), torch.zeros(6, dtype=torch.bool), 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        osh_counts(torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.bool), 10)
    lut, counts = torch.rand(30, 256), torch.zeros(1, 2, 30, dtype=torch.int32)
    w, b = torch.zeros(1, 256), torch.zeros(1)
    for kw in (dict(max_epochs=0), dict(max_epochs=1_000_001)):
        with pytest.raises(ValueError):
            fit_hyperplanes_counts(lut, counts, 15, w, b, **kw)
    with pytest.raises(ValueError):
        fit_hyperplanes_counts(lut, counts, 0, w, b)
    with pytest.raises(ValueError):
        fit_hyperplanes_counts(torch.rand(30, 1025), counts, 15, torch.zeros(1, 1025), b)
    with pytest.raises(ValueError):
        fit_hyperplanes_counts(lut, torch.zeros(1, 2, 29, dtype=torch.int32), 15, w, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit_hyperplanes_counts(lut, counts, 15, w, b)


# ---- the direct cases (tests/osh_reference.py: DIRECT_CASES) ---------------------------------------------------------------
def test_direct_case_table_covers_the_kernel_shapes():
    shapes = {(c["n_codes"], c["D"]): c["frac"] for c in DIRECT_CASES.values() if "counts" not in c}
    want = {(1, 1): 1, (1, 256): 1, (5, 63): 1, (15, 256): 1, (16, 64): 1, (17, 65): 1, (40, 256): 0.3, (319, 256): 1,
            (320, 256): 1, (321, 256): 1, (1000, 256): 0.31, (1000, 1024): 1, (1000, 1000): 0.5, (999, 33): 1, (640, 512): 1,
            (37, 100): 1}
    assert shapes == want
    for (n, d) in want:
        eps = {c["epochs"] for c in DIRECT_CASES.values() if (c["n_codes"], c["D"]) == (n, d)}
        assert eps == ({1, 8, 64} if n <= 320 else {1, 8}), (n, d)
    big = [c for c in DIRECT_CASES.values() if "counts" in c]
    assert {c["epochs"] for c in big} == {1, 8, 64}
    for c in big:
        assert (c["n_codes"], c["D"], c["HW"]) == (3, 64, 2 ** 31 - 1) and int(np.sum(c["counts"])) == c["HW"]
    assert all(c["HW"] == 4096 for c in DIRECT_CASES.values() if "counts" not in c)


def test_direct_case_presence_is_interleaved():
    """The sparse cases have absent codes between present ones, the compaction ends where the table says, and every
    case's counts sum to HW."""
    for name, m_max, m_min in (("40x256_e1", 15, 1), ("1000x256_e1", 400, 250), ("1000x1000_e1", 600, 400)):
        case = direct_case(name)
        present = case["counts"].sum(0) > 0
        assert m_min <= present.sum() <= m_max, name
        runs = int((np.diff(present.astype(int)) != 0).sum())  # boundaries between present and absent stretches
        assert runs >= max(1, present.sum() // 4), name
    for name in ("1000x1024_e1", "999x33_e1", "320x256_e1", "17x65_e1"):
        assert (direct_case(name)["counts"].sum(0) > 0).all(), name
    for name in DIRECT_CASES:
        case = direct_case(name)
        assert case["counts"].sum() == case["HW"] and case["counts"].min() >= 0, name


@pytest.mark.parametrize("name", sorted(DIRECT_CASES))
def test_direct_case_is_far_from_every_kink(name):
    """The kink guard: the float64 fit's smallest distance of a margin to {-1, 0, 1} is at least 32 times the largest
    margin error of the case's own fp32 restatement, which therefore shows no IoU flip -- and runs the stated epochs."""
    case = direct_case(name)
    r64, r32 = reference_fits(case)
    assert r64["epochs"] == r32["epochs"] == case["epochs"]
    assert r64["kink"] == kink_of(r64["margins"])
    assert r64["kink"] >= GUARD_FACTOR * margin_error(r64, r32), (r64["kink"], margin_error(r64, r32))
    assert iou_flips(r64["trace"][:, 1], r32["trace"][:, 1]) == 0
    assert r64["init_iou"] == r32["init_iou"] and not np.isnan(r64["trace"][:, 1]).any()
    tol = direct_tolerances(r64, r32)
    assert all(0 < t < 1e-4 * s for t, s in ((tol["w"], np.abs(r64["w"]).max()), (tol["trace"], r64["trace"][:, 0].max())))


@pytest.mark.parametrize("shape", KINK_SHAPES)
@pytest.mark.parametrize("b0", KINK_B0)
def test_kink_case_sits_on_the_kink_and_leaves_it(shape, b0):
    """w0 = 0: every margin of the first pass is b0 exactly, in both precisions; the margins after the one step pass the
    guard."""
    case = kink_case(shape, b0)
    r64, r32 = reference_fits(case)
    assert (r64["margins"][0] == b0).all() and (r32["margins"][0] == b0).all()
    assert kink_of(r64["margins"][1:]) >= GUARD_FACTOR * margin_error(r64, r32, first=1)
    assert iou_flips(r64["trace"][:, 1], r32["trace"][:, 1]) == 0
    P, N = case["counts"].astype(np.float64)
    HW = case["HW"]
    want_init = P.sum() / HW if b0 > 0 else 0.0        # everything predicted / nothing predicted (positives exist)
    assert P.sum() > 0 and r64["init_iou"] == r32["init_iou"] == want_init
    want_loss = {1.0: 2 * N.sum(), -1.0: 2 * P.sum(), 0.0: HW}[b0] / HW
    assert r64["trace"][0, 0] == pytest.approx(want_loss, rel=1e-12)
    # both hinges pass their gradient at the kink: b moves by -lr (N - P) / HW
    assert r64["b"] == pytest.approx(b0 - 0.01 * (N.sum() - P.sum()) / HW, rel=1e-12)
