"""The fixed-budget densification on the device (csrc/mcmc.hip, goi_hyperplane_amd/mcmc.py) against its numpy restatement
(tests/mcmc_reference.py) on every named case (tests/mcmc_cases.py), then through the model: no host synchronisation, the
composite preserved end to end, and growth into a pad at a constant P.

Integers (counts, hit counts, copied rows, zeroed moments) are compared exactly.  The new opacities and log-scales are held to
the restatement's float64 value rounded to fp32 within ONE ulp(fp32): the device's float64 pow / log / exp differ from numpy's by
a few 1e-16 relative, against a half-ulp of 6e-8, so a result can move by at most one rounding step.  The relocation sum D has only
+, * and table values: bit-equal.  The noise: the same margin by the same derivation (exp, sqrt and the divisions in float64)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import densify_reference as dref
from tests import mcmc_cases as mc
from tests import mcmc_reference as ref

pytestmark = pytest.mark.gpu
CASES = mc.cases()
MODES = {"opacity": ref.OPACITY, "scaling": ref.SCALING}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import _lib
    return _lib.load()


def groups_of(c, params, moments):
    """[(label, array, mode)] in the order the Python layer hands the groups over"""
    out = []
    for n in mc.NAMES:
        if params[n].shape[1] == 0:
            continue
        out.append((n, params[n], MODES.get(n, ref.PARAM)))
        if n in moments:
            out += [(n + ".exp_avg", moments[n][0], ref.MOMENT), (n + ".exp_avg_sq", moments[n][1], ref.MOMENT)]
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    c = CASES[name]
    groups = groups_of(c, *mc.tensors(c))
    r = ref.relocate(c["opacity"], c["draws"], c["selection"], c["min_opacity"], c["max_moves"], c["frac"], c["n_max"],
                     [(a, m) for _, a, m in groups])
    return groups, r


def ordered(a):
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def within_one_ulp(got, want64):
    want = np.asarray(want64, np.float64).astype(np.float32)
    return bool((np.abs(ordered(got) - ordered(want)) <= 1).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_entry(lib, dev, c, groups, hits=True):
    """one goi_mcmc_relocate call on fresh device copies: ({label: array}, counts, hits, status, inputs after the call)"""
    from goi_hyperplane_amd import _lib
    P = c["P"]
    t = [torch.from_numpy(a.copy()).to(dev) for _, a, _ in groups]
    opacity = torch.from_numpy(c["opacity"].copy()).to(dev)
    draws = torch.tensor(c["draws"], dtype=torch.int64, device=dev)
    sel = None if c["selection"] is None else torch.from_numpy(c["selection"].copy()).to(dev)
    counts = torch.full((4,), -7, dtype=torch.int32, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    h = torch.full((P,), -7, dtype=torch.int32, device=dev) if hits else None
    ws = _lib.workspace(lib.goi_mcmc_relocate_workspace_bytes(P), dev)
    arr = (_lib.GoiMcmcRows * len(groups))(*[_lib.GoiMcmcRows(x.data_ptr(), int(a.shape[1]), m) for x, (_, a, m) in zip(t, groups)])
    r = lib.goi_mcmc_relocate(P, _lib.ptr(opacity), _lib.ptr(draws), len(c["draws"]), _lib.ptr(sel), c["min_opacity"], c["max_moves"],
                              c["frac"][0], c["frac"][1], c["n_max"], arr, len(groups), _lib.ptr(h), _lib.ptr(counts), _lib.ptr(status),
                              _lib.ptr(ws), _lib.stream(dev))
    assert r == 0, _lib.last_error()
    torch.cuda.synchronize(dev)
    out = {label: x.cpu().numpy() for x, (label, _, _) in zip(t, groups)}
    after = (opacity.cpu().numpy(), draws.cpu().tolist(), None if sel is None else sel.cpu().numpy())
    return out, counts.cpu().tolist(), None if h is None else h.cpu().tolist(), int(status.item()), after


def check_against_reference(c, groups, r, out, counts, hits, status):
    assert status == 0
    assert counts == r["counts"]
    assert hits == r["hits"]
    written = sorted(set(r["dead"][:r["moves"]]) | set(r["values"]))
    for (label, old, mode), want in zip(groups, r["groups"]):
        got = out[label]
        if mode in (ref.PARAM, ref.MOMENT):
            assert np.array_equal(bits(got), bits(want)), label  # copies bit-equal, source moments zero, the rest untouched
            continue
        rest = np.setdiff1d(np.arange(c["P"]), written)
        assert np.array_equal(bits(got[rest]), bits(old[rest])), label
        w64 = r["opacity64"] if mode == ref.OPACITY else r["scale64"]
        for i in r["values"]:
            assert within_one_ulp(got[i], w64[i]), (label, i, got[i], w64[i])
        for j, s in enumerate(r["src"]):
            assert np.array_equal(bits(got[r["dead"][j]]), bits(got[s])), (label, j)  # a copy carries its source's new bits


@pytest.mark.parametrize("name", [n for n in CASES if n != "p0"])
def test_relocate_entry_on_every_case(lib, dev, name):
    c = CASES[name]
    groups, r = reference(name)
    out, counts, hits, status, after = run_entry(lib, dev, c, groups)
    print(name, "counts", counts, "max r", max(hits, default=0))
    check_against_reference(c, groups, r, out, counts, hits, status)
    assert np.array_equal(bits(after[0]), bits(c["opacity"])) and after[1] == c["draws"]
    assert (after[2] is None) if c["selection"] is None else np.array_equal(after[2], c["selection"])
    # the same bits on a second call, the hit counts kept in the workspace this time
    out2, counts2, _, status2, _ = run_entry(lib, dev, c, groups, hits=False)
    assert counts2 == counts and status2 == 0
    for label in out:
        assert np.array_equal(bits(out[label]), bits(out2[label])), label


def test_p_zero_touches_nothing(lib, dev):
    c = CASES["p0"]
    groups, _ = reference("p0")
    out, counts, hits, status, _ = run_entry(lib, dev, c, groups)
    assert counts == [-7] * 4 and status == -7 and hits == []


def test_a_draw_out_of_range_raises_its_status_bit(lib, dev):
    c = dict(CASES["p2"])
    c["draws"] = [123456789 + (1 << 32), 1]
    groups, r = reference("p2")
    out, counts, hits, status, _ = run_entry(lib, dev, c, groups)
    assert status == 1 and counts == r["counts"] and hits == r["hits"]  # the low 32 bits were used


def test_rows_permuted_together_with_the_targets_give_the_same_rows_as_sets(lib, dev):
    """p257 with every dead row moved (moves == n_dead): the rows are permuted, and each draw gets the smallest u whose target
    falls into its source's interval at the source's new place.  Then every source is hit as often as before, so every group holds
    the same multiset of rows: the alive rows, r copies of each source's row, the sources' new values, the zeroed moments."""
    name = "p257"
    c = CASES[name]
    groups, r = reference(name)
    assert r["moves"] == r["counts"][1] > 0
    rng = np.random.default_rng(99)
    perm = rng.permutation(c["P"])  # new row k holds old row perm[k]
    where = np.argsort(perm)        # old row i sits at where[i]
    cp = dict(c)
    cp["opacity"] = c["opacity"][perm]
    s0 = ref.sample(cp["opacity"], [], None, c["min_opacity"], 0, c["frac"])
    T = s0["T"]
    assert T == r["T"]
    draws = []
    for s in r["src"]:
        k = int(where[s])
        lo = s0["C"][k - 1] if k else 0
        draws.append(-((-lo << 32) // T))  # ceil(lo * 2^32 / T): the smallest u with floor(u T / 2^32) >= lo
    cp["draws"] = draws
    gp = [(label, a[perm], m) for label, a, m in groups]
    rp = ref.relocate(cp["opacity"], cp["draws"], None, c["min_opacity"], c["max_moves"], c["frac"], c["n_max"], [(a, m) for _, a, m in gp])
    assert rp["src"] == [int(where[s]) for s in r["src"]]
    out, counts, hits, status, _ = run_entry(lib, dev, c, groups)
    outp, countsp, hitsp, statusp, _ = run_entry(lib, dev, cp, gp)
    assert counts == countsp and statusp == 0 and [hitsp[int(where[i])] for i in range(c["P"])] == hits
    for label in out:
        assert sorted(row.tobytes() for row in out[label]) == sorted(row.tobytes() for row in outp[label]), label


def test_relocation_sum_is_bit_equal_to_the_restatement(lib, dev):
    from goi_hyperplane_amd import _lib
    pairs = [(v["o_new"], v["N"]) for name in ("p5000", "one_alive_300_dead", "opaque", "n_max_3", "interleaved")
             for v in reference(name)[1]["values"].values()]
    for o in (0.0051, 0.5, 0.95, 1 - 2.0 ** -10, 1 - 2.0 ** -16, 1 - 2.0 ** -20, 1 - 2.0 ** -24):
        for N in (1, 2, 5, 13, 30, 40, 51):
            pairs.append((ref.new_values(np.float32(o), N, mc.MIN_OP)[1], N))
    o_new = torch.tensor([p[0] for p in pairs], dtype=torch.float64, device=dev)
    N = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=dev)
    D = torch.empty_like(o_new)
    assert lib.goi_mcmc_debug_relocation_sum(len(pairs), _lib.ptr(o_new), _lib.ptr(N), _lib.ptr(D), _lib.stream(dev)) == 0, _lib.last_error()
    want = np.array([ref.relocation_sum(o, n) for o, n in pairs], np.float64)
    assert np.array_equal(D.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert {n for _, n in pairs} >= {2, 3, 51}


# ---- the noise ---------------------------------------------------------------------------------------------------------------------

NOISE_CASES = ("p1_alive", "p2", "p63", "p64", "p65", "p257", "p5000", "frozen_dead", "opaque", "threshold")
STEP = 5e5 * 1.6e-4


@pytest.mark.parametrize("name", NOISE_CASES)
def test_noise_entry(lib, dev, name):
    """Frozen rows are bit-unchanged.  The stated case of the gate: at step = 80 (5e5 x 1.6e-4) a row with opacity >= 0.5 has
    g <= exp(-100 * 0.495) = 3e-22, its move is below 1e-19 for scales below 1 and |z| < 10 -- far below half an ulp of any
    position above 1e-12 -- so it is bit-unchanged too."""
    from goi_hyperplane_amd import _lib
    c = CASES[name]
    P = c["P"]
    params, _ = mc.tensors(c, seed=3)
    op = np.nan_to_num(c["opacity"], nan=0.3).astype(np.float32)
    z = np.random.default_rng(5).standard_normal((P, 3)).astype(np.float32)
    sel = c["selection"]
    want = ref.noise(params["xyz"], params["rotation"], params["scaling"], op, z, sel, 100.0, 0.995, STEP)
    t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in (("xyz", params["xyz"]), ("rot", params["rotation"]), ("scal", params["scaling"]),
                                                            ("op", op), ("z", z))}
    tsel = None if sel is None else torch.from_numpy(sel.copy()).to(dev)
    assert lib.goi_mcmc_noise(P, _lib.ptr(t["xyz"]), _lib.ptr(t["rot"]), _lib.ptr(t["scal"]), _lib.ptr(t["op"]), _lib.ptr(t["z"]),
                              _lib.ptr(tsel), 100.0, 0.995, STEP, _lib.stream(dev)) == 0, _lib.last_error()
    got = t["xyz"].cpu().numpy()
    assert within_one_ulp(got, want)
    moved = (bits(got) != bits(params["xyz"])).any(axis=1)
    if sel is not None:
        assert not moved[sel == 0].any() and moved[(sel != 0) & (op < 0.01)].any()
    assert not moved[op >= 0.5].any()
    if (op < 0.004).any():
        assert moved[(op < 0.004) & (sel != 0 if sel is not None else True)].all()  # g > 0.5 there: transparent rows do move
    for k, v in (("rot", params["rotation"]), ("scal", params["scaling"]), ("op", op), ("z", z)):
        assert np.array_equal(bits(t[k].cpu().numpy()), bits(v)), k


# ---- through the model -------------------------------------------------------------------------------------------------------------

def model(dev, P=600, seed=3, dead=0.25, optimizer="fused"):
    m = dref.make_model(P, dev, seed=seed, optimizer=optimizer)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        kill = (torch.rand(P, 1, generator=g) < dead).to(dev)
        m._opacity.copy_(torch.where(kill, torch.full_like(m._opacity, -7.0), m._opacity.clamp(min=-3.0)))
    return m


def model_groups(m):
    out = []
    for n, attr in dref.PARAMS:
        p = getattr(m, attr)
        out.append((n, p.detach().reshape(p.shape[0], -1).cpu().numpy().copy(), MODES.get(n, ref.PARAM)))
        st = m.optimizer.state[p]
        out += [(n + "." + k, st[k].reshape(p.shape[0], -1).cpu().numpy().copy(), ref.MOMENT) for k in ("exp_avg", "exp_avg_sq")]
    return out


def test_relocate_and_add_noise_never_synchronise_and_keep_every_object(dev):
    from goi_hyperplane_amd import mcmc
    m = model(dev)
    P = m._xyz.shape[0]
    mcmc.relocate(model(dev, seed=4), generator=torch.Generator(device=dev).manual_seed(1))  # loads the library, warms the allocator
    opacity = torch.sigmoid(m._opacity.detach()).reshape(P).cpu().numpy()
    groups = model_groups(m)
    stats = {k: getattr(m, k).clone() for k in dref.STATS}
    objects = {attr: getattr(m, attr) for _, attr in dref.PARAMS}
    states = {attr: m.optimizer.state[p] for attr, p in objects.items()}
    versions = {attr: p._version for attr, p in objects.items()}
    mversions = {attr: st["exp_avg"]._version for attr, st in states.items()}
    sel = torch.ones(P, dtype=torch.bool, device=dev)
    sel[::7] = False
    gen = torch.Generator(device=dev).manual_seed(11)
    draws = torch.randint(0, 2 ** 32, (P,), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(11))
    z = torch.empty((P, 3), dtype=torch.float32, device=dev).normal_(0.0, 1.0, generator=torch.Generator(device=dev).manual_seed(12))
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        counts = mcmc.relocate(m, selection=sel, generator=gen)
        xyz_mid = m._xyz.detach().clone()
        mcmc.add_noise(m, 1.6e-4, selection=sel, generator=torch.Generator(device=dev).manual_seed(12))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert counts.is_cuda and counts.dtype == torch.int32 and int(mcmc.status().item()) == 0
    r = ref.relocate(opacity, draws.cpu().tolist(), sel.cpu().numpy().astype(np.uint8), 0.005, 1 << 30, mc.NO_LIMIT, 51,
                     [(a, mode) for _, a, mode in groups])
    assert counts.cpu().tolist() == r["counts"] and r["moves"] > 50
    for attr, p in objects.items():
        assert getattr(m, attr) is p and isinstance(p, torch.nn.Parameter) and p._version > versions[attr], attr
        assert m.optimizer.state[p] is states[attr] and states[attr]["exp_avg"]._version > mversions[attr], attr
    assert [g["params"][0] for g in m.optimizer.param_groups] == [objects[attr] for _, attr in dref.PARAMS]
    got = {label: a for label, a, _ in model_groups(m)}
    got["xyz"] = xyz_mid.cpu().numpy()
    c = {"P": P}
    check_against_reference(c, groups, r, got, counts.cpu().tolist(), r["hits"], 0)
    for k, v in stats.items():
        assert torch.equal(getattr(m, k), v), k  # the statistics are not touched
    # the noise moved the selected transparent rows from where the relocation left them, and only those it may
    want = ref.noise(xyz_mid.cpu().numpy(), m._rotation.detach().cpu().numpy(), m._scaling.detach().cpu().numpy(),
                     torch.sigmoid(m._opacity.detach()).reshape(P).cpu().numpy(), z.cpu().numpy(), sel.cpu().numpy(), 100.0, 0.995, STEP)
    assert within_one_ulp(m._xyz.detach().cpu().numpy(), want)
    assert torch.equal(m._xyz.detach()[::7], xyz_mid[::7])


def test_relocation_preserves_the_composite_and_the_rasterizers_state(dev):
    """One Gaussian of opacity 0.9 on the centre of pixel (16, 16) of a 32 x 32 view and 7 dead ones elsewhere.  After relocate the
    8 coincide with o' = 1 - 0.1^(1/8) = 0.25 (well above the 1/255 cut), and the alpha at that pixel is what it was, within the
    forward gate of 1e-4 of the parity suite."""
    import math
    from goi_hyperplane_amd import _C, mcmc
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera
    m = dref.make_model(8, dev, seed=2, optimizer="fused", steps=1)
    x = (2 * 16 + 1 - 32) / 32 * 5.0 * math.tan(0.5)  # pixel centre 16 of 32 at depth 5
    with torch.no_grad():
        m._xyz.copy_(torch.tensor([[x, x, 0.0]] + [[-0.8 + 0.1 * i, 0.9, 0.2] for i in range(7)], device=dev))
        m._opacity.copy_(torch.tensor([[math.log(0.9 / 0.1)]] + [[-20.0]] * 7, device=dev))
        m._scaling.fill_(math.log(0.3))
        m._rotation.copy_(torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 8, device=dev))
    cam = TorchCamera(make_camera(32, 32), dev)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        before = render(cam, m, PipelineParams(), bg)["alpha"].reshape(32, 32)[16, 16].item()
    state = _C._spec_state(dev)
    seen_P = state.get("P")
    objects = {attr: getattr(m, attr) for _, attr in dref.PARAMS}
    versions = {attr: p._version for attr, p in objects.items()}
    counts = mcmc.relocate(m, generator=torch.Generator(device=dev).manual_seed(0))
    assert counts.cpu().tolist() == [7, 7, 1, 1]
    assert torch.equal(m._xyz.detach(), m._xyz.detach()[:1].expand(8, 3))
    o_new = torch.sigmoid(m._opacity.detach())
    assert torch.equal(o_new, o_new[:1].expand(8, 1)) and abs(o_new[0].item() - (1 - 0.1 ** 0.125)) < 1e-6
    assert (m._scaling.detach() < math.log(0.3)).all()
    with torch.no_grad():
        after = render(cam, m, PipelineParams(), bg)["alpha"].reshape(32, 32)[16, 16].item()
    print("alpha before", before, "after", after)
    assert abs(before - 0.9) < 1e-4 and abs(after - before) <= 1e-4
    assert _C._spec_state(dev) is state and state.get("P") == seen_P
    for attr, p in objects.items():
        assert getattr(m, attr) is p and p._version > versions[attr], attr


def test_pad_then_growth_by_five_percent_at_a_constant_p(dev):
    from goi_hyperplane_amd import mcmc
    m = dref.make_model(400, dev, seed=6, optimizer="fused")
    with torch.no_grad():
        m._opacity.clamp_(min=-2.0)  # all 400 alive: sigmoid(-2) = 0.12
    old = {attr: getattr(m, attr).detach().clone() for _, attr in dref.PARAMS}
    old_m = {attr: m.optimizer.state[getattr(m, attr)]["exp_avg"].clone() for _, attr in dref.PARAMS}
    mcmc.pad(m, 1000)
    for name, attr in dref.PARAMS:
        p = getattr(m, attr)
        assert p.shape[0] == 1000 and isinstance(p, torch.nn.Parameter) and p.requires_grad
        assert torch.equal(p.detach()[:400], old[attr])
        st = m.optimizer.state[p]
        assert torch.equal(st["exp_avg"][:400], old_m[attr]) and not st["exp_avg"][400:].any() and not st["exp_avg_sq"][400:].any()
        assert [g for g in m.optimizer.param_groups if g["name"] == name][0]["params"][0] is p
        if attr == "_opacity":
            assert (p.detach()[400:] == -20.0).all()
        elif attr == "_rotation":
            assert torch.equal(p.detach()[400:], torch.tensor([1.0, 0, 0, 0], device=dev).expand(600, 4))
        else:
            assert torch.equal(p.detach()[400:], old[attr][:1].expand((600,) + tuple(old[attr].shape[1:])))
    assert m.xyz_gradient_accum.shape == (1000, 1) and m.denom.shape == (1000, 1) and m.max_radii2D.shape == (1000,)
    assert not m.xyz_gradient_accum[400:].any() and not m.max_radii2D[400:].any()
    assert len(m.optimizer.state) == 7
    objects = {attr: getattr(m, attr) for _, attr in dref.PARAMS}
    gen = torch.Generator(device=dev).manual_seed(21)
    alive, seen = 400, []
    for _ in range(3):
        counts = mcmc.relocate(m, max_fraction=(1, 20), generator=gen).cpu().tolist()
        seen.append(counts)
        assert counts[:3] == [alive // 20, 1000 - alive, alive]
        alive += alive // 20
    assert [c[0] for c in seen] == [20, 21, 22] and alive == 463
    assert int((torch.sigmoid(m._opacity.detach()) > 0.005).sum()) == 463
    for attr, p in objects.items():
        assert getattr(m, attr) is p and p.shape[0] == 1000
    m.optimizer.zero_grad(set_to_none=True)
    for _, attr in dref.PARAMS:
        getattr(m, attr).grad = torch.zeros_like(getattr(m, attr))
    m.optimizer.step()  # the optimizer still steps on the same keys
