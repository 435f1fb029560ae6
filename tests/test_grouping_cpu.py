"""The closed-form gradient of the mask-contrast loss against float64 autograd of its definition, the numpy restatement
(tests/grouping_reference.py) on every case of tests/grouping_cases.py, and goi_hyperplane_amd.grouping's argument checks.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import grouping_cases as gc
from tests import grouping_reference as ref

CHECKED = [n for n in gc.names() if n != "max_abs_exceeded"]  # (a saturated sum is not the definition's)


def _kw(c):
    return {k: v for k, v in c["kw"].items() if k != "max_abs"}


def _closed_form(feat, labels, K, margin=1.0, w_intra=1.0, w_inter=1.0, balance="pixel"):
    """dL/df_p = alpha_m f_p + beta_m with the float64 means of the features themselves -> (loss, grad)"""
    S, H, W = feat.shape
    lab = labels.reshape(-1).astype(np.int64)
    ok = (lab >= 0) & (lab < K)
    f = feat.reshape(S, -1).T.astype(np.float64)
    n = np.bincount(lab[ok], minlength=K)[:K].astype(np.float64) if K else np.zeros(0)
    live = n > 0
    M, N = int(live.sum()), n.sum()
    mu = np.zeros((K, S))
    np.add.at(mu, lab[ok], f[ok])
    mu[live] /= n[live][:, None]
    a = np.zeros(K)
    if M:
        a[live] = 1.0 / N if balance == "pixel" else 1.0 / (M * n[live])
    g, inter = np.zeros((K, S)), 0.0
    for m in np.flatnonzero(live) if M > 1 else ():
        for o in np.flatnonzero(live):
            if o == m:
                continue
            d = np.sqrt(((mu[m] - mu[o]) ** 2).sum())
            inter += (margin * margin if d == 0 else max(0.0, margin - d) ** 2) / (M * (M - 1))
            if 0 < d < margin:
                g[m] += -4.0 / (M * (M - 1)) * (margin - d) / d * (mu[m] - mu[o])
    alpha = 2.0 * w_intra * a
    beta = -alpha[:, None] * mu + w_inter * g / np.maximum(n, 1)[:, None]
    grad = np.zeros_like(f)
    grad[ok] = alpha[lab[ok], None] * f[ok] + beta[lab[ok]]
    intra = (a[lab[ok]] * ((f[ok] - mu[lab[ok]]) ** 2).sum(-1)).sum()
    return w_intra * intra + w_inter * inter, np.ascontiguousarray(grad.T).reshape(S, H, W)


@pytest.mark.parametrize("name", CHECKED)
def test_the_closed_form_gradient_equals_float64_autograd_of_the_definition(name):
    c = gc.case(name)
    want_loss, want = ref.definition(c["feat"], c["labels"], c["K"], **_kw(c))
    loss, grad = _closed_form(c["feat"], c["labels"], c["K"], **_kw(c))
    # alpha f + beta cancels |f| against |mu|: float64 rounding of the offset, not of the gradient
    top, big = float(np.abs(c["feat"]).max()), float(np.abs(want).max())
    assert np.abs(grad - want).max() <= 1e-12 * max(1.0, top) * big + 1e-300, name
    assert abs(loss - want_loss) <= 1e-11 * max(abs(want_loss), 1e-300) + 1e-18


def test_the_case_list_covers_every_bullet():
    covered = set().union(*(c["tags"] for c in gc.cases()))
    assert covered == set(gc.TAGS), sorted(set(gc.TAGS) ^ covered)
    assert {c["feat"].shape[0] for c in gc.cases()} >= {1, 3, 16, 17, 32}
    assert {c["feat"].shape[1:] for c in gc.cases()} >= {(1, 1), (1, 63), (1, 64), (1, 65), (7, 9), (16, 16), (37, 53), (129, 65), (256, 256)}
    assert {c["K"] for c in gc.cases()} >= {0, 1, 2, 5, 300, 4096}
    for c in gc.cases():
        assert c["feat"].dtype == np.float32 and c["labels"].dtype == np.int32 and c["feat"].shape[1:] == c["labels"].shape
        assert c["feat"].shape[1] * c["feat"].shape[2] <= 140_000, "tests stay quick"
    r = gc.reference("odd_K300")
    assert r["M"] == 12 and (r["count"] == 0).sum() == 288
    assert gc.reference("big_cells")["count"][39] == 1
    assert gc.reference("all_ignored")["M"] == 0 and gc.reference("K0")["M"] == 0
    r = gc.reference("twins")
    assert np.array_equal(r["qsum"][0], r["qsum"][1]) and r["count"][0] == r["count"][1] == 64
    r = gc.reference("at_margin")
    assert np.array_equal(r["mu"], [[0, 0, 0], [1, 0, 0], [5, 0, 0]]) and not r["g"].any() and r["inter"] == 0.0
    assert gc.reference("zeros")["qexp"] == 40 and gc.reference("max_abs_exceeded")["status"] == 1
    assert len(set(gc.case("tall_random64")["labels"][0, :64].tolist())) > 32  # (nearly) every lane another label
    assert np.abs(gc.case("offset_1000")["feat"]).min() > 990


@pytest.mark.parametrize("name", CHECKED)
def test_the_restatement_against_the_definition(name):
    """the integer sums are the counts and, to half a quantum per pixel, the float64 sums; loss and gradient are the definition's
    up to what half a quantum in every mean can move them (nothing near a kink: the cases at d == 0 and d == margin are exact)"""
    c = gc.case(name)
    r = gc.reference(name)
    S = c["feat"].shape[0]
    lab = c["labels"].reshape(-1).astype(np.int64)
    ok = (lab >= 0) & (lab < c["K"])
    assert r["status"] == 0 and r["count"].dtype == r["qsum"].dtype == np.int64
    assert np.array_equal(r["count"], np.bincount(lab[ok], minlength=c["K"])[:c["K"]] if c["K"] else np.zeros(0, np.int64))
    top = float(np.abs(c["feat"]).max()) if "max_abs" not in c["kw"] else c["kw"]["max_abs"]
    e = 40 - r["qexp"]
    assert top < 2.0 ** e and (top == 0 or top >= 2.0 ** (e - 1))
    exact = np.zeros((c["K"], S))
    np.add.at(exact, lab[ok], c["feat"].reshape(S, -1).T.astype(np.float64)[ok])
    unit = 2.0 ** -r["qexp"]
    assert np.all(np.abs(r["qsum"] * unit - exact) <= 0.5 * unit * r["count"][:, None] + 1e-12 * np.abs(exact))
    assert np.abs(r["qsum"]).max(initial=0) < 2 ** 62
    want_loss, want = ref.definition(c["feat"], c["labels"], c["K"], **_kw(c))
    near = 2.0 ** (e - 36)  # half a quantum in every mean, with room for the pair terms' slopes
    assert abs(r["loss"] - want_loss) <= near * max(1.0, abs(want_loss))
    assert np.abs(r["grad"] - want).max() <= near * max(1.0, float(np.abs(want).max())) * 64
    assert not r["grad"].reshape(S, -1)[:, ~ok].any()


def test_the_float32_twin_is_a_float32_computation_near_the_restatement():
    for name in ("big_cells", "offset_1000", "tall_random64"):
        t, r = gc.twin(name), gc.reference(name)
        assert t["grad"].dtype == np.float32 and isinstance(t["loss"], np.float32)
        assert abs(float(t["loss"]) - r["loss"]) <= 1e-3 * max(abs(r["loss"]), 1e-6)
        assert 0 < np.abs(t["grad"] - r["grad"]).max() <= 2e-2 * np.abs(r["grad"]).max()


# ---- the module's argument checks ----------------------------------------------------------------------------------------------------
def test_the_module_is_exported_and_lazy():
    import goi_hyperplane_amd
    from goi_hyperplane_amd import grouping
    assert goi_hyperplane_amd.grouping is grouping and "grouping" in goi_hyperplane_amd.__all__
    for name in ("loss", "loss_terms", "FeatureView", "fit", "instances"):
        assert callable(getattr(grouping, name))


def test_argument_checks_without_a_gpu():
    from goi_hyperplane_amd import grouping
    f, l = torch.zeros(4, 5, 6), torch.zeros(5, 6, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grouping.loss(f, l, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grouping.loss_terms(f, l, 0)
    with pytest.raises(TypeError, match="feat must be a tensor"):
        grouping.loss(f.numpy(), l, 3)
    with pytest.raises(TypeError, match="feat must be float32"):
        grouping.loss(f.double(), l, 3)
    with pytest.raises(TypeError, match="labels must be int32"):
        grouping.loss(f, l.long(), 3)
    for bad in (torch.zeros(5, 6), torch.zeros(0, 5, 6), torch.zeros(33, 5, 6), torch.zeros(4, 0, 6)):
        with pytest.raises(ValueError, match=r"feat must have shape \(S, H, W\)"):
            grouping.loss(bad, l, 3)
    with pytest.raises(ValueError, match=r"labels must have shape \(5, 6\)"):
        grouping.loss(f, torch.zeros(6, 5, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match=r"H \* W <= 2\^22"):
        grouping.loss(torch.zeros(1, 2049, 2048), torch.zeros(2049, 2048, dtype=torch.int32), 3)
    with pytest.raises(TypeError, match="K must be an int"):
        grouping.loss(f, l, 3.0)
    with pytest.raises(TypeError, match="K must be an int"):
        grouping.loss(f, l, True)
    for bad in (-1, 2 ** 16 + 1):
        with pytest.raises(ValueError, match="0 <= K <= 65536"):
            grouping.loss(f, l, bad)
    with pytest.raises(ValueError, match="balance must be 'pixel' or 'mask'"):
        grouping.loss(f, l, 3, balance="both")
    for kw in (dict(margin=-1.0), dict(margin=float("nan")), dict(margin=float("inf")), dict(max_abs=-0.5), dict(max_abs=float("inf"))):
        with pytest.raises(ValueError, match="need a finite .* >= 0"):
            grouping.loss(f, l, 3, **kw)
    for kw in (dict(w_intra=float("nan")), dict(w_inter=float("inf"))):
        with pytest.raises(ValueError, match="need a finite w_"):
            grouping.loss(f, l, 3, **kw)


def test_feature_view_and_fit_checks_without_a_gpu():
    from goi_hyperplane_amd import grouping

    class Model:
        get_xyz = torch.zeros(7, 3, requires_grad=True)
        get_scaling = get_rotation = get_opacity = get_features = torch.ones(7, 3, requires_grad=True)
        get_semantics = torch.zeros(7, 16)
        active_sh_degree = 2

    pc, feats = Model(), torch.zeros(7, 4)
    view = grouping.FeatureView(pc, feats)
    assert view.get_semantics is feats and view.get_xyz is pc.get_xyz and view.active_sh_degree == 2
    frozen = grouping.FeatureView(pc, feats, frozen=True)
    assert frozen.get_semantics is feats and not frozen.get_xyz.requires_grad and frozen.get_xyz is frozen.get_xyz
    assert frozen.get_xyz.data_ptr() == pc.get_xyz.data_ptr() and not frozen.get_opacity.requires_grad
    with pytest.raises(AttributeError):
        view.no_such_thing
    with pytest.raises(ValueError, match=r"features must have shape \(P, S\)"):
        grouping.FeatureView(pc, torch.zeros(6, 4))
    with pytest.raises(ValueError, match="one label map per camera"):
        grouping.fit([object()], pc, [], 2)
    with pytest.raises(ValueError, match="1 <= S <= 32"):
        grouping.fit([object()], pc, [torch.zeros(2, 2, dtype=torch.int32)], 2, S=33)
    with pytest.raises(ValueError, match="iterations"):
        grouping.fit([object()], pc, [torch.zeros(2, 2, dtype=torch.int32)], 2, iterations=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grouping.fit([object()], pc, [torch.zeros(2, 2, dtype=torch.int32)], 2)
