"""CPU checks of the fixed-budget densification (goi_hyperplane_amd/mcmc.py, csrc/mcmc.hip): the numpy restatement
(tests/mcmc_reference.py) against exact arithmetic and against the properties the algorithm promises, the coverage of the case
list (tests/mcmc_cases.py), and the Python layer's refusals.  The device code is held to the restatement in
tests/test_gpu_mcmc.py."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import densify_reference as dref
from tests import mcmc_cases as mc
from tests import mcmc_reference as ref

O_GRID = (0.0051, 0.5, 0.95, 1 - 2.0 ** -10, 1 - 2.0 ** -16, 1 - 2.0 ** -20, 1 - 2.0 ** -24)
N_GRID = (1, 2, 5, 13, 30, 40, 51)
# 1 / sqrt(k + 1) to 100 decimal digits as a rational: isqrt(10^200 / (k + 1)) / 10^100
Q_EXACT = [Fraction(math.isqrt(10 ** 200 // (k + 1)), 10 ** 100) for k in range(ref.N_MAX)]


def exact_sum(o_new, N):
    x = Fraction(o_new)  # the float64 the restatement works from, exactly
    D = Fraction(0)
    for m in range(1, N + 1):
        for k in range(m):
            D += math.comb(m - 1, k) * (-1) ** k * Q_EXACT[k] * x ** (k + 1)
    return D


@pytest.mark.parametrize("o", O_GRID)
@pytest.mark.parametrize("N", N_GRID)
def test_relocation_sum_against_exact_arithmetic(o, N):
    """The float64 chain of the restatement (and of the kernel, which is held to it bit for bit) within 1e-9 relative of the
    sum in rational arithmetic -- a condition.  Worst on this grid: 1.2e-12 at o = 1 - 2^-24, N = 51; an fp32 chain reaches
    2e-4, which is why the sum is float64."""
    _, o_new, D, _, _ = ref.new_values(np.float32(o), N, mc.MIN_OP)
    exact = exact_sum(o_new, N)
    err = abs(Fraction(D) - exact) / exact
    print(f"o={o!r} N={N} rel err {float(err):.3e}")
    assert err <= Fraction(1, 10 ** 9)


def test_tables_are_exact():
    assert all(ref.BINOM[n][k] == math.comb(n, k) for n in range(51) for k in range(51))
    assert math.comb(50, 25) < 2 ** 53
    assert all(abs(Fraction(ref.Q[k]) - Q_EXACT[k]) * 2 ** 53 <= 1 for k in range(51))  # one rounding of a value below 1


@pytest.mark.parametrize("o", O_GRID + (1.0,))
def test_one_copy_changes_nothing(o):
    o32 = np.float32(o)
    oc, o_new, D, c, _ = ref.new_values(o32, 1, mc.MIN_OP)
    assert oc == min(float(o32), 1 - 2.0 ** -24) and o_new == oc and D == oc and c == 1.0 and math.log(c) == 0.0


@pytest.mark.parametrize("o", O_GRID)
@pytest.mark.parametrize("N", N_GRID)
def test_copies_compose_to_the_source_opacity(o, N):
    """1 - (1 - o')^N = o to 1e-12 absolute: o' carries one rounding of pow and one of the subtraction (2^-53 each, values
    below 1), N copies multiply that by at most N = 51: 2e-14."""
    oc, o_new, _, _, _ = ref.new_values(np.float32(o), N, mc.MIN_OP)
    assert abs(Fraction(1) - (1 - Fraction(o_new)) ** N - Fraction(oc)) <= Fraction(1, 10 ** 12)


@pytest.fixture(scope="module")
def sampled():
    return {name: (c, ref.sample(c["opacity"], c["draws"], c["selection"], c["min_opacity"], c["max_moves"], c["frac"], c["n_max"]))
            for name, c in mc.cases().items()}


def test_sampling_invariants_on_every_case(sampled):
    for name, (c, s) in sampled.items():
        C = s["C"]
        assert all(a <= b for a, b in zip(C, C[1:])), name
        assert s["T"] == (C[-1] if C else 0) == sum(s["w"]), name
        assert all(s["alive"][i] and s["w"][i] > 0 for i in s["src"]), name
        assert sum(s["hits"]) == s["moves"] == len(s["src"]), name
        assert s["moves"] <= min(len(s["dead"]), len(c["draws"]), c["max_moves"]), name
        assert not set(s["dead"]) & set(s["src"]), name
        assert s["dead"] == sorted(s["dead"]), name
        if c["selection"] is not None:
            frozen = set(np.flatnonzero(c["selection"] == 0).tolist())
            assert not frozen & (set(s["dead"]) | set(s["src"])), name


def test_source_frequencies_follow_the_weights():
    """200 000 draws over 50 alive rows: Pearson's X^2 = sum (n_i - n p_i)^2 / (n p_i), p_i = w_i / T, has 49 degrees of freedom.
    Laurent and Massart's bound P(X^2 >= k + 2 sqrt(k x) + 2 x) <= exp(-x) with k = 49, x = 20 (2e-9) gives 151.6; every expected
    count is above 400, so the chi-square limit holds.  The sampler's own bias is nil at this scale: row i owns w_i > 8e4
    consecutive targets and each target receives floor or ceil(2^32 / T) of the 2^32 values of u, so p_i is off by at most one
    value of u in w_i * 2^32 / T of them (below 2e-6 relative)."""
    rng = np.random.default_rng(2024)
    op = np.concatenate((rng.random(50) * 0.9 + 0.05, np.full(10, 0.001))).astype(np.float32)
    op = op[rng.permutation(60)]
    n = 200_000
    w, _, alive = ref.classify(op, None, mc.MIN_OP)
    C = np.cumsum(np.asarray(w, np.uint64))
    T = int(C[-1])
    u = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    # the restatement's rule on integers that fit: u * T < 2^32 * 2^30
    t = (u * np.uint64(T)) >> np.uint64(32)
    src = np.searchsorted(C, t, side="right")  # min{ i : C_i > t }
    probe = ref.sample(op, u[:500].tolist(), None, mc.MIN_OP, 500, mc.NO_LIMIT)
    assert probe["moves"] == 10 and probe["src"] == src[:10].tolist()  # the vectorised rule is the restatement's
    counts = np.bincount(src, minlength=60)
    expect = n * np.asarray(w, np.float64) / T
    assert counts[~alive].sum() == 0 and expect[alive].min() > 400
    x2 = float((((counts - expect) ** 2)[alive] / expect[alive]).sum())
    print("X^2 =", x2)
    assert x2 <= 49 + 2 * math.sqrt(49 * 20) + 2 * 20


def test_the_case_list_covers_what_was_specified(sampled):
    cs = {n: c for n, (c, _) in sampled.items()}
    ss = {n: s for n, (_, s) in sampled.items()}
    assert {c["P"] for c in cs.values()} >= {0, 1, 2, 63, 64, 65, 257, 5000}
    assert {c["rest"] for c in cs.values()} == {0, 45} and {c["S"] for c in cs.values()} == {1, 16}
    assert ss["no_dead"]["counts"][1] == 0 and ss["no_dead"]["moves"] == 0
    assert ss["all_dead"]["T"] == 0 and ss["all_dead"]["counts"][:3] == [0, 64, 0]
    assert max(ss["one_alive_300_dead"]["hits"]) == 300 and ss["one_alive_300_dead"]["counts"] == [300, 300, 1, 1]
    assert ss["n_max_3"]["moves"] == 300
    d = ss["dead_block"]["dead"]
    assert d == list(range(100, 140))
    assert ss["u_zero"]["src"] and set(ss["u_zero"]["src"]) == {min(i for i, w in enumerate(ss["u_zero"]["w"]) if w)}
    assert set(ss["u_max"]["src"]) == {max(i for i, w in enumerate(ss["u_max"]["w"]) if w)}
    b = ss["boundaries"]
    alive = [1, 2, 5, 8, 9, 13, 20, 23]
    assert b["T"] == 1 << 26 and b["src"][:14] == [alive[n - 1 + k] for n in range(1, 8) for k in (0, 1)]
    nd = ss["p257"]["counts"][1]
    assert len(cs["more_draws"]["draws"]) > nd > len(cs["fewer_draws"]["draws"]) > 0
    assert ss["more_draws"]["moves"] == nd and ss["fewer_draws"]["moves"] == len(cs["fewer_draws"]["draws"])
    assert [ss[k]["moves"] for k in ("max_moves_0", "max_moves_1", "max_moves_below", "max_moves_above")] == [0, 1, nd - 1, nd]
    assert ss["frac_to_0"]["moves"] == 0 and ss["frac_to_1"]["moves"] == 1
    assert ss["frac_5_percent"]["moves"] == ss["frac_5_percent"]["counts"][2] // 20 > 0
    t = cs["threshold"]
    assert float(t["opacity"][3]) == mc.MIN_OP and 3 in ss["threshold"]["dead"] and ss["threshold"]["alive"][4]
    assert t["opacity"][4] == np.nextafter(np.float32(mc.MIN_OP), np.float32(1))
    assert any(cs["opaque"]["opacity"][i] == 1.0 for i in ss["opaque"]["src"]) and ss["opaque"]["T"] == 3 << 24
    n = ss["nan"]
    assert np.isnan(cs["nan"]["opacity"][[0, 7, 64]]).all() and not {0, 7, 64} & (set(n["dead"]) | set(n["src"]))
    assert n["counts"][1] + n["counts"][2] == 62
    f = cs["frozen_dead"]
    assert f["opacity"][2] < mc.MIN_OP and f["selection"][2] == 0 and 2 not in ss["frozen_dead"]["dead"]
    assert ss["frozen_only_source"]["T"] == 0 and ss["frozen_only_source"]["counts"] == [0, 9, 0, 0]
    assert 0 < len(cs["moments_some"]["moments"]) < 7 and cs["moments_none"]["moments"] == ()
    assert any(max(s["hits"], default=0) >= 2 for s in ss.values())


def test_restated_rows(sampled):
    """the restatement on one case, by hand: copies are the source's rows, the source's moments are zero, everything else stays"""
    c, _ = sampled["p65"]
    params, moments = mc.tensors(c)
    groups, names = [], []
    for n in mc.NAMES:
        if params[n].shape[1]:
            groups.append((params[n], {"opacity": ref.OPACITY, "scaling": ref.SCALING}.get(n, ref.PARAM)))
            names.append(n)
            if n in moments:
                groups += [(moments[n][0], ref.MOMENT), (moments[n][1], ref.MOMENT)]
                names += [n + ".m", n + ".v"]
    r = ref.relocate(c["opacity"], c["draws"], c["selection"], c["min_opacity"], c["max_moves"], c["frac"], c["n_max"], groups)
    new = dict(zip(names, r["groups"]))
    touched = set(r["dead"][:r["moves"]]) | set(r["values"])
    for j, s in enumerate(r["src"]):
        d = r["dead"][j]
        assert (new["xyz"][d] == params["xyz"][s]).all() and (new["rotation"][d] == params["rotation"][s]).all()
        assert new["opacity"][d] == new["opacity"][s] and (new["scaling"][d] == new["scaling"][s]).all()
        assert (new["xyz.m"][s] == 0).all() and (new["xyz.m"][d] == moments["xyz"][0][d]).all()
        assert (new["scaling"][s] < params["scaling"][s]).all() or r["values"][s]["c"] >= 1.0
    rest = [i for i in range(c["P"]) if i not in touched]
    for n, (a, _) in zip(names, groups):
        assert (new[n][rest] == a[rest]).all(), n


# ---- the Python layer's refusals (no GPU: the checks that come before any device work) ---------------------------------------

def cpu_model(P=8):
    return dref.make_model(P, "cpu", optimizer=None)


def test_refusals_of_relocate():
    from goi_hyperplane_amd import mcmc
    g = cpu_model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mcmc.relocate(g)
    for bad in (1.5, "3", True):
        with pytest.raises(TypeError, match="max_moves must be an int or None"):
            mcmc.relocate(g, max_moves=bad)
    with pytest.raises(ValueError, match="max_moves must be >= 0"):
        mcmc.relocate(g, max_moves=-1)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"min_opacity must be in \[0, 1\)"):
            mcmc.relocate(g, min_opacity=bad)
    for bad in (0.05, (1,), (1.0, 20), (1, 2, 3), (True, 2)):
        with pytest.raises(TypeError, match="max_fraction must be a pair of integers"):
            mcmc.relocate(g, max_fraction=bad)
    for bad in ((-1, 20), (1, 0), (2 ** 32 + 1, 1), (1, 2 ** 32 + 1)):
        with pytest.raises(ValueError, match="max_fraction needs"):
            mcmc.relocate(g, max_fraction=bad)
    for bad in ([1, 2], torch.zeros(4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(TypeError, match="draws must be a 1-D torch.int64 tensor"):
            mcmc.relocate(g, draws=bad)
    g._xyz = torch.nn.Parameter(g._xyz.detach().double())
    with pytest.raises(TypeError, match="_xyz must be torch.float32"):
        mcmc.relocate(g)
    g = cpu_model()
    g.set_semantic_masks(torch.ones(8))
    with pytest.raises(ValueError, match="semantic mask"):
        mcmc.relocate(g)


def test_refusals_of_add_noise_and_pad():
    from goi_hyperplane_amd import mcmc
    g = cpu_model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mcmc.add_noise(g, 1.6e-4)
    for kw in ({"noise_lr": float("inf")}, {"k": float("nan")}, {"x0": float("-inf")}):
        with pytest.raises(ValueError, match="must be finite"):
            mcmc.add_noise(g, 1.6e-4, **kw)
    with pytest.raises(ValueError, match="must be finite"):
        mcmc.add_noise(g, float("nan"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mcmc.pad(g, 16)
    for bad in (16.0, "16", True, None):
        with pytest.raises(TypeError, match="budget must be an int"):
            mcmc.pad(g, bad)


def test_regularisers_are_the_papers_mean_absolute_terms():
    from goi_hyperplane_amd import mcmc
    g = cpu_model(33)
    assert torch.equal(mcmc.opacity_regulariser(g), torch.sigmoid(g._opacity).abs().mean())
    assert torch.equal(mcmc.scale_regulariser(g), torch.exp(g._scaling).abs().mean())
    (mcmc.opacity_regulariser(g) + mcmc.scale_regulariser(g)).backward()
    assert g._opacity.grad is not None and g._scaling.grad is not None
