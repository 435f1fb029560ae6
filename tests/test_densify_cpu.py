"""CPU checks of goi_hyperplane_amd.densify and of the densification semantics in tests/densify_reference.py.

* the restatement is the reference's own GaussianModel methods bit for bit (tests/golden/ref_densify_pins.npz):
  densify_and_prune with the recorded normal draws, with and without max_screen_size, prune_points, reset_opacity;
* the restatement's final layout: originals kept, clones, first children, second children, each in ascending original
  index; clones and children carry zero moments, kept rows their own; `step` untouched; statistics zeroed;
* the host refuses CPU tensors (no fallback), a model with a semantic mask, and a missing 2-D mean gradient."""
import pytest
import torch
from torch import nn

from goi_hyperplane_amd import densify
from tests import densify_reference as ref


def test_restated_layout_and_moments():
    m = ref.make_model(300, "cpu", seed=2)
    raw = {attr: getattr(m, attr).detach().clone() for _, attr in ref.PARAMS}
    moments = {name: (m.optimizer.state[getattr(m, attr)]["exp_avg"].clone(),
                      float(m.optimizer.state[getattr(m, attr)]["step"])) for name, attr in ref.PARAMS}
    info = ref.densify_and_prune(m, 2e-4, 0.1, 4.0, None, generator=torch.Generator().manual_seed(1))
    K, C, S = info["kept"], info["clones"], info["children"]
    assert K > 0 and C > 0 and S > 0
    assert m._xyz.shape[0] == K + C + 2 * S
    # the kept originals are a subsequence of the input in ascending order; clones copy rows raw
    sem = raw["_semantics"]
    idx = [int((sem == row).all(dim=1).nonzero()[0]) for row in m._semantics.detach()]
    assert idx[:K] == sorted(idx[:K]) and idx[K:K + C] == sorted(idx[K:K + C])
    assert idx[K + C:K + C + S] == idx[K + C + S:] == sorted(idx[K + C:K + C + S])
    for _, attr in ref.PARAMS:
        if attr not in ("_xyz", "_scaling"):
            assert torch.equal(getattr(m, attr).detach(), raw[attr][idx])
    assert torch.equal(m._scaling.detach()[:K + C], raw["_scaling"][idx[:K + C]])
    for name, attr in ref.PARAMS:
        st = m.optimizer.state[getattr(m, attr)]
        assert m.optimizer.param_groups[[g["name"] for g in m.optimizer.param_groups].index(name)]["params"][0] is getattr(m, attr)
        assert torch.equal(st["exp_avg"][:K], moments[name][0][idx[:K]])
        assert not bool(st["exp_avg"][K:].any()) and not bool(st["exp_avg_sq"][K:].any())
        assert float(st["step"]) == moments[name][1]
    for name in ref.STATS:
        assert not bool(getattr(m, name).any()) and getattr(m, name).shape[0] == K + C + 2 * S


def test_restated_prune_without_optimizer_or_statistics():
    m = ref.make_model(50, "cpu", seed=3, optimizer=None)
    m.xyz_gradient_accum = torch.empty(0)
    m.denom = torch.empty(0)
    mask = torch.arange(50) % 3 == 0
    ref.prune_points(m, mask)
    assert m._xyz.shape[0] == 50 - int(mask.sum()) and m.max_radii2D.shape[0] == m._xyz.shape[0]
    assert m.denom.numel() == 0 and isinstance(m._xyz, nn.Parameter)


def test_host_refuses():
    m = ref.make_model(10, "cpu", seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        densify.prune_points(m, torch.zeros(10, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        densify.densify_and_prune(m, 2e-4, 0.1, 4.0, None)
    m.set_semantic_masks(torch.ones(10))
    with pytest.raises(ValueError, match="semantic mask"):
        densify.prune_points(m, torch.zeros(10, dtype=torch.bool))
    vp = torch.zeros(10, 3, requires_grad=True)
    with pytest.raises(ValueError, match="accumulate mode"):
        densify.add_densification_stats(m, vp, torch.ones(10, dtype=torch.bool))


def _assert_bits(got, want, what):
    import numpy as np
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got.view(np.int32) != want.view(np.int32)
    assert not diff.any(), (what, int(diff.sum()), float(np.abs(got.astype(np.float64) - want).max()))


def _assert_outputs(m, d, case):
    got, want = ref.model_outputs(m), ref.pinned_outputs(d, case)
    for k in want:
        _assert_bits(got[k], want[k], f"{case}: {k}")
    for name, attr in ref.PARAMS:  # each group holds the model's new tensor, re-keyed
        group = next(g for g in m.optimizer.param_groups if g["name"] == name)
        assert group["params"][0] is getattr(m, attr) and isinstance(getattr(m, attr), nn.Parameter)


@pytest.mark.parametrize("case,max_screen_size", [("dp_none", None), ("dp_screen", 20)])
def test_restatement_is_the_reference_bit_for_bit(case, max_screen_size):
    """densify_and_prune of tests/densify_reference.py against the reference's own clone -> split -> prune-parents -> prune
    sequence (tests/golden/ref_densify_pins.npz) with the recorded standard-normal draws: rows, order, values, both
    moments and `step` of all 7 groups, and the zeroed statistics, bit for bit."""
    d = ref.pins()
    m = ref.pins_model(d, "cpu")
    z = torch.from_numpy(d[f"{case}_z"].copy())
    info = ref.densify_and_prune(m, float(d["max_grad"]), float(d["min_opacity"]), float(d["extent"]), max_screen_size,
                                 normal=lambda mean, std: z * std + mean)
    _assert_outputs(m, d, case)
    P, n_split = int(d["P"]), z.shape[0] // 2
    # the pins hold a real mix: clones, split children, pruned originals, 0/0 and x/0 statistics, and with
    # max_screen_size the world-size prune on top
    assert info["clones"] > 0 and info["children"] > 0 and info["kept"] + n_split < P
    assert ((d["in_denom"] == 0) & (d["in_xyz_gradient_accum"] == 0)).any()
    assert ((d["in_denom"] == 0) & (d["in_xyz_gradient_accum"] > 0)).any()
    if max_screen_size:
        assert d["dp_screen_xyz"].shape[0] < d["dp_none_xyz"].shape[0]


def test_restated_prune_points_and_reset_opacity_are_the_reference_bit_for_bit():
    d = ref.pins()
    m = ref.pins_model(d, "cpu")
    ref.prune_points(m, torch.from_numpy(d["prune_mask"].copy()))
    _assert_outputs(m, d, "prune")
    m = ref.pins_model(d, "cpu")
    ref.reset_opacity(m)
    _assert_outputs(m, d, "reset")
