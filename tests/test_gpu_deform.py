"""goi_hyperplane_amd.deform on the GPU against tests/deform_reference.py (float64: the reference; float32: the twin).

  1. sample_nodes: ids, order and count equal the numpy restatement;
  2. solve: y and q (up to sign) within max(8 x the float32 twin's error, 64 ulps of the case's coordinate scale) of the float64
     reference after 1, 2 and 25 iterations, the energy within max(8 x the twin's error, 64 ulps of the energy itself);
     iterations = 0 returns the warm start;
  3. apply: the same rule per tensor, every SH band separately against edit.sh_rotation(R_g) @ c in float64; rows that take no part
     keep their bits;
  4. identity in, the same bits out; reset() restores the model bit for bit;
  5. a rigid motion of every node agrees with edit.transform within the sum of the two paths' bounds, moments included;
  6. the same bits on a second call and with the unselected rows scrambled;
  7. solve, energy, apply and commit never synchronise; exactly the tensors written have their version bumped;
  8. a bar of 2000 Gaussians, one end pinned, the other turned by 90 degrees, end to end.

The twin's error is computed here from the two numpy runs, never from the kernel."""
import numpy as np
import pytest
import torch
from torch import nn

from goi_hyperplane_amd import deform, edit, knn, smooth
from tests import deform_cases as cases
from tests import deform_reference as ref
from tests import densify_reference as dref
from tests import edit_reference as eref

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
ULPS = 64
MARGIN = 8  # the project's margin over the twin's own error (tests/test_gpu_grouping.py, tests/test_gpu_pca.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def t(a, dev, dtype=None):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=dev).contiguous()


def host(x):
    return x.detach().cpu().numpy().copy()


def within(got, want64, twin, scale, what):
    """max(8 x the twin's error, 64 ulps of `scale`); prints the figures before it asserts"""
    want64 = np.asarray(want64, np.float64)
    e_twin = float(np.abs(np.asarray(twin, np.float64) - want64).max()) if want64.size else 0.0
    err = float(np.abs(np.asarray(got, np.float64) - want64).max()) if want64.size else 0.0
    tol = max(MARGIN * e_twin, ULPS * EPS * scale)
    print(f"{what}: err {err:.3e} twin {e_twin:.3e} tol {tol:.3e}")
    assert err <= tol, what


def align(q, like):
    """q with every row's sign chosen to agree with `like` (q and -q are one rotation)"""
    s = np.where((np.asarray(q, np.float64) * like).sum(axis=1) < 0, -1.0, 1.0)
    return np.asarray(q, np.float64) * s[:, None]


def snapshot(g):
    out = {attr: host(getattr(g, attr)) for _, attr in dref.PARAMS}
    if getattr(g, "optimizer", None) is not None:
        for grp in g.optimizer.param_groups:
            for k, v in (g.optimizer.state.get(grp["params"][0], None) or {}).items():
                out[f"{grp['name']}.{k}"] = host(v) if torch.is_tensor(v) else np.asarray(v)
    return out


# ---- 1. sample_nodes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 2000])
def test_sample_nodes_equals_the_restatement(dev, P):
    xyz = cases.bar(P, 30 + P)
    half = np.random.default_rng(P).random(P) < 0.5
    for name, sel, inv, eff in (("none", None, False, None), ("half", half, False, half), ("inverted", half, True, ~half),
                                ("empty", np.zeros(P, bool), False, np.zeros(P, bool)), ("bytes", half.astype(np.uint8) * 7, False, half)):
        for spacing in (0.3, 10.0):
            got = deform.sample_nodes(t(xyz, dev), t(sel, dev), spacing, invert=inv)
            want = ref.sample_nodes(xyz, eff, spacing)
            assert got.dtype == torch.int64 and np.array_equal(host(got), want), (name, spacing)
            if spacing == 10.0 and want.size:
                assert want.size == 1  # one cube holds the whole bar: its lowest selected id


# ---- 2. the solve -----------------------------------------------------------------------------------------------------------------
def gpu_solve(c, dev, iterations, **kw):
    con = t(c["constrained"], dev)
    y, q = deform.solve(t(c["x"], dev), t(c["idx"], dev), con, t(c["target"], dev), weight=t(c["weight"], dev), y0=t(c["y0"], dev),
                        q0=t(c["q0"], dev), iterations=iterations, **kw)
    return y, q


def energy_tol(E64, E32):
    """max(8 x the twin's error, 64 float32 ulps of the energy itself)"""
    return max(MARGIN * abs(E32 - E64), ULPS * EPS * abs(E64))


@pytest.mark.parametrize("c", cases.solve_cases(), ids=lambda c: c["name"])
def test_solve_is_within_the_twin_margin_of_float64(dev, c):
    x, idx, w = c["x"], c["idx"], c["weight"]
    scale = float(max(np.abs(x).max(), np.abs(c["target"]).max() if c["target"] is not None else 0.0))
    for it in (1, 2, 25):
        kw = dict(y0=c["y0"], q0=c["q0"], iterations=it)
        y64, q64 = ref.solve(x, idx, w, c["constrained"], c["target"], dtype=np.float64, **kw)
        y32, q32 = ref.solve(x, idx, w, c["constrained"], c["target"], dtype=np.float32, **kw)
        y, q = gpu_solve(c, dev, it)
        within(host(y), y64, y32, scale, f"{c['name']} it {it} y")
        within(align(host(q), q64), q64, align(q32, q64), 1.0, f"{c['name']} it {it} q")
        assert np.abs(np.linalg.norm(host(q).astype(np.float64), axis=1) - 1).max() < 8 * EPS  # (a normalised fp32 quaternion is within about 4 eps)
        E64, E32 = ref.energy(x, idx, w, y64, q64), ref.energy(x, idx, w, y32, q32)
        E = float(deform.energy(t(x, dev), t(idx, dev), y, q, t(w, dev)))
        tol = energy_tol(E64, E32)
        print(f"{c['name']} it {it} E: got {E:.6e} want {E64:.6e} twin {E32:.6e} tol {tol:.3e}")
        assert abs(E - E64) <= tol
        # the energy entry itself, on the twin's own y and q: float64 terms, so only the order of the sum differs
        E_twin = float(deform.energy(t(x, dev), t(idx, dev), t(y32, dev), t(q32, dev), t(w, dev)))
        assert abs(E_twin - E32) <= 1e-12 * max(E32, 1e-30)
        if c["constrained"] is not None:
            pinned = c["constrained"].astype(bool)
            assert same_bits(host(y)[pinned], c["target"][pinned])


def test_zero_iterations_return_the_warm_start_and_the_transpose_may_be_handed_in(dev):
    c = next(c for c in cases.solve_cases() if c["name"].startswith("bend60_warm"))
    y, q = gpu_solve(c, dev, 0)
    assert same_bits(host(y), c["y0"]) and same_bits(host(q), c["q0"])
    y1, q1 = gpu_solve(c, dev, 3)
    y2, q2 = gpu_solve(c, dev, 3, transposed=smooth.transpose(t(c["idx"], dev)))
    assert same_bits(host(y1), host(y2)) and same_bits(host(q1), host(q2))
    ya, qa = gpu_solve(c, dev, 2)  # 2 + 1 iterations from the warm start it returned = 3 iterations
    yb, qb = deform.solve(t(c["x"], dev), t(c["idx"], dev), t(c["constrained"], dev), t(c["target"], dev), y0=ya, q0=qa, iterations=1)
    assert same_bits(host(yb), host(y1)) and same_bits(host(qb), host(q1))


# ---- 3. the apply -----------------------------------------------------------------------------------------------------------------
def gpu_apply(c, dev, scramble=False):
    """-> (before, after, bind, effective mask) with the model tensors as numpy arrays"""
    P = len(c["xyz"])
    nx, ny, nq = c["nodes"]
    mask = c["mask"]
    rows = np.ones(P, bool) if mask is None else mask
    xyz, rot, rest = c["xyz"].copy(), c["rot"].copy(), c["rest"].copy()
    if scramble:
        rng = np.random.default_rng(5)
        for a in (xyz, rot, rest):
            a[~rows] = rng.normal(size=a[~rows].shape).astype(np.float32)
    if P and len(nx):
        bind = knn.query(t(c["xyz"], dev), t(nx, dev), c["kb"], query_mask=t(mask, dev))
    else:
        bind = (torch.full((P, c["kb"]), -1, dtype=torch.int32, device=dev), torch.full((P, c["kb"]), np.inf, device=dev))
    if c["name"].startswith("P2000") and rows.any():  # a selected row without a node
        bind[0][int(np.nonzero(rows)[0][0])] = -1
    sel, inv = (None, False) if mask is None else ((~mask, True) if c["inverted"] else (mask, False))
    src = tuple(t(a, dev) for a in (xyz, rot, rest))
    dst = tuple(a.clone() for a in src)
    deform.apply_nodes(dst, src, bind, (t(nx, dev), t(ny, dev), t(nq, dev)), c["sigma"], t(sel, dev), invert=inv)
    return (xyz, rot, rest), tuple(host(a) for a in dst), (host(bind[0]), host(bind[1])), rows


@pytest.mark.parametrize("c", cases.apply_cases(), ids=lambda c: c["name"])
def test_apply_is_within_the_twin_margin_of_float64(dev, c):
    before, after, bind, rows = gpu_apply(c, dev)
    a64 = ref.apply(*before, *bind, c["nodes"], c["sigma"], rows, np.float64, "host")
    a32 = ref.apply(*before, *bind, c["nodes"], c["sigma"], rows, np.float32, "lane")
    part = rows & ((bind[0] >= 0) & np.isfinite(bind[1])).any(axis=1)
    if c["name"].startswith("P2000"):
        assert (rows & ~part).sum() == 1
    if c["name"].endswith("few_nodes"):
        assert (bind[0][part] == -1).any()  # -1 tails: fewer nodes than kb
    for got, was in zip(after, before):
        assert same_bits(got[~part], was[~part]), c["name"]
    if not part.any():
        return
    scale = float(max(np.abs(before[0]).max(), np.abs(c["nodes"][1]).max()))
    within(after[0][part], a64[0][part], a32[0][part], scale, f"{c['name']} xyz")
    within(after[1][part], a64[1][part], a32[1][part], float(np.abs(a64[1]).max()), f"{c['name']} rotation")
    nb = before[2].shape[1]
    for l in (1, 2, 3):
        lo, hi = l * l - 1, (l + 1) * (l + 1) - 1
        if hi <= nb:
            within(after[2][part, lo:hi], a64[2][part, lo:hi], a32[2][part, lo:hi], float(np.abs(a64[2][:, lo:hi]).max()),
                   f"{c['name']} band {l}")
    if c["name"].endswith("identity"):
        for got, was in zip(after, before):
            assert same_bits(got, was)
    elif not np.array_equal(a64[0].astype(np.float32), before[0]):  # (one Gaussian on the identity node does not move)
        assert not same_bits(after[0], before[0])


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------
def test_the_same_bits_on_a_second_call_and_with_the_unselected_rows_scrambled(dev):
    c = next(c for c in cases.apply_cases() if c["name"].startswith("P2000"))
    _, first, _, rows = gpu_apply(c, dev)
    _, second, _, _ = gpu_apply(c, dev)
    _, third, _, _ = gpu_apply(c, dev, scramble=True)
    for a, b, s in zip(first, second, third):
        assert same_bits(a, b)
        assert same_bits(a[rows], s[rows])
    s = next(c for c in cases.solve_cases() if c["name"].startswith("hostile"))
    (y1, q1), (y2, q2) = gpu_solve(s, dev, 25), gpu_solve(s, dev, 25)
    assert same_bits(host(y1), host(y2)) and same_bits(host(q1), host(q2))
    e = [float(deform.energy(t(s["x"], dev), t(s["idx"], dev), y1, q1, t(s["weight"], dev))) for _ in range(2)]
    assert e[0] == e[1]


# ---- the session ------------------------------------------------------------------------------------------------------------------
def bar_model(dev, P=2000, M=16, S=16, seed=3, optimizer="adam"):
    g = dref.make_model(P, dev, seed=seed, M=M, S=S, optimizer=optimizer)
    with torch.no_grad():
        g._xyz.copy_(t(cases.bar(P, seed, length=2.0, width=0.25) - np.float32([1.0, 0.0, 0.0]), dev))
    return g


def half_selection(P, dev, seed=1):
    return (torch.rand(P, generator=torch.Generator().manual_seed(seed)) < 0.5).to(dev)


# ---- 4. identity and reset --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", ["none", "half", "inverted", "empty"])
def test_identity_in_is_bit_identity_out_and_reset_restores_the_model(dev, sel):
    g = bar_model(dev)
    half = half_selection(2000, dev)
    selection, inv = {"none": (None, False), "half": (half, False), "inverted": (half, True),
                      "empty": (torch.zeros(2000, dtype=torch.bool, device=dev), False)}[sel]
    before = snapshot(g)
    d = deform.Deformation(g, selection, spacing=0.2, invert=inv)
    if sel == "empty":
        assert d.M == 0
    d.constrain(torch.arange(min(d.M, 5)), d.x[:min(d.M, 5)])  # pinned where they are: nothing is displaced
    d.solve(iterations=5).apply()
    after = snapshot(g)
    for k in before:
        assert same_bits(after[k], before[k]), k
    if d.M:
        d.drag(d.x[:, 0] > 0.5, rotation=cases.axis_angle((0, 0, 1), 40.0), translation=(0.0, 0.2, 0.0)).solve(iterations=10).apply()
        moved = snapshot(g)
        eff = np.ones(2000, bool) if selection is None else (host(selection) != inv)
        for k in before:
            changed = k in ("_xyz", "_rotation", "_features_rest")
            assert same_bits(moved[k], before[k]) != changed, k
            if moved[k].ndim:  # (Adam's `step` is a scalar)
                assert same_bits(moved[k][~eff], before[k][~eff]), k
        d.reset()
        assert float(d.energy()) == 0.0
    after = snapshot(g)
    for k in before:
        assert same_bits(after[k], before[k]), k


# ---- 5. agreement with the rigid path ---------------------------------------------------------------------------------------------
def test_a_rigid_motion_of_every_node_agrees_with_edit_transform(dev):
    kw = dict(rotation=eref.random_rotation(21), translation=(0.3, -0.2, 0.1), pivot=(0.1, 0.2, -0.1))
    P = 2000
    a, b = bar_model(dev, P), bar_model(dev, P)
    sel = half_selection(P, dev)
    eff = host(sel)
    before = snapshot(a)
    d = deform.Deformation(a, sel, spacing=0.2)
    d.drag(torch.arange(d.M), **kw).solve(iterations=25).apply()
    qg = None
    rest = tuple(host(r) for r in d.rest)
    bind = (host(d.bind[0]), host(d.bind[1]))
    nodes_x, idx, target = host(d.x), host(d.idx), host(d.target)
    d.commit()
    edit.transform(b, sel, scale=1.0, **kw)
    got_a, got_b = snapshot(a), snapshot(b)
    # the float64 reference of both paths: the rigid motion itself
    arrays = {k: before[k] for k in ("_xyz", "_rotation", "_scaling", "_features_rest")}
    for name, _attr, key in eref.MOMENTS:
        arrays[key] = before[f"{name}.exp_avg"]
    want = eref.transform({k: v.astype(np.float64) for k, v in arrays.items()}, eff, eref.constants(dtype=np.float64, **kw))
    twin_b = eref.transform(arrays, eff, eref.constants(dtype=np.float32, **kw))
    # the twin of the deformation path: the float32 restatement of the solve from the targets drag() set, then of the apply
    con = np.ones(len(nodes_x), np.uint8)
    y32, q32 = ref.solve(nodes_x, idx, None, con, target, iterations=25, dtype=np.float32)
    x32, r32, c32, qg, turn = ref.apply(*rest, *bind, (nodes_x, y32, q32), d.sigma, eff, np.float32, "lane")
    mx, mr, mc = ref.turn_moments(arrays["m_xyz"], arrays["m_rotation"], arrays["m_features_rest"], qg, turn, np.float32, "lane")
    twin_a = {"_xyz": x32, "_rotation": r32, "_features_rest": c32, "m_xyz": mx, "m_rotation": mr, "m_features_rest": mc}
    keys = {"_xyz": "_xyz", "_rotation": "_rotation", "_features_rest": "_features_rest", "m_xyz": "xyz.exp_avg",
            "m_rotation": "rotation.exp_avg", "m_features_rest": "f_rest.exp_avg"}
    # q_g and -q_g are one rotation: where the blend chose the other sign than edit's q_R, the raw quaternion AND its moment come out
    # negated together (still one consistent Adam state); both are compared up to that one sign per row
    def signed(rot, arrays_):
        s = np.where((rot.astype(np.float64) * want["_rotation"]).sum(axis=1) < 0, -1.0, 1.0).astype(np.float32)[:, None]
        return {k: (v * s if k in ("_rotation", "m_rotation") else v) for k, v in arrays_.items()}

    twin_a = signed(twin_a["_rotation"], twin_a)
    got_a.update({keys[k]: v for k, v in signed(got_a["_rotation"], {k: got_a[snap] for k, snap in keys.items()}).items()})
    for key, snap in keys.items():
        w = want[key][eff]
        scale = float(np.abs(w).max())
        bound = sum(max(MARGIN * float(np.abs(tw[key][eff].astype(np.float64) - w).max()), ULPS * EPS * scale) for tw in (twin_a, twin_b))
        err = float(np.abs(got_a[snap][eff].astype(np.float64) - got_b[snap][eff]).max())
        print(f"rigid {key}: deform vs edit {err:.3e}, bound {bound:.3e}")
        assert err <= bound, key
        assert same_bits(got_a[snap][~eff], before[snap][~eff]), key
    for k in before:  # exp_avg_sq, step, every other group and parameter: as edit.transform leaves them
        if k not in keys.values():
            assert same_bits(got_a[k], before[k]), k


# ---- 7. no host synchronisation, version counters ---------------------------------------------------------------------------------
def test_solve_apply_and_commit_never_synchronise_and_bump_exactly_what_they_write(dev):
    g = bar_model(dev)
    sel = half_selection(2000, dev)
    d = deform.Deformation(g, sel, spacing=0.2)
    handle = torch.nonzero(d.x[:, 0] > 0.5).squeeze(1)
    q = torch.tensor(cases.axis_angle((1, 0, 0), 30.0), dtype=torch.float32)
    params = {attr: getattr(g, attr) for _, attr in dref.PARAMS}
    moments = {f"{grp['name']}.{k}": v for grp in g.optimizer.param_groups for k, v in g.optimizer.state[grp["params"][0]].items()
               if torch.is_tensor(v)}
    d.drag(handle, rotation=q, pivot=(1.0, 0.0, 0.0))  # (host numbers go to the device here: not part of the claim)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d.solve(iterations=3)
        e = d.energy()
        v0 = {k: v._version for k, v in {**params, **moments}.items()}
        d.apply()
        v1 = {k: v._version for k, v in {**params, **moments}.items()}
        d.commit()
        v2 = {k: v._version for k, v in {**params, **moments}.items()}
        d.solve(iterations=1).apply()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert float(e) > 0
    for k in v0:
        assert (v1[k] > v0[k]) == (k in ("_xyz", "_rotation", "_features_rest")), k
        assert (v2[k] > v1[k]) == (k in ("xyz.exp_avg", "rotation.exp_avg", "f_rest.exp_avg")), k


def test_node_ids_out_of_range_raise_on_the_host_and_are_ignored_on_the_device(dev):
    g = bar_model(dev, P=300, optimizer=None)
    d = deform.Deformation(g, spacing=0.2)
    for bad in ([-1], [d.M], torch.tensor([0, d.M])):
        with pytest.raises(ValueError, match="node ids"):
            d.constrain(bad, (0.0, 0.0, 0.0))
    ids = torch.tensor([-1, d.M, 2, 10 ** 9], device=dev)
    d.constrain(ids, torch.arange(12, dtype=torch.float32, device=dev).view(4, 3))
    con = host(d.constrained)
    assert con.sum() == 1 and con[2] == 1 and np.array_equal(host(d.target)[2], np.float32([6, 7, 8]))
    assert same_bits(np.delete(host(d.target), 2, axis=0), np.delete(host(d.x), 2, axis=0))
    d.drag(ids, translation=(1.0, 0.0, 0.0))
    assert np.allclose(host(d.target)[2], host(d.x)[2] + np.float32([1, 0, 0]), atol=1e-6) and host(d.constrained).sum() == 1
    d.release(ids)
    assert host(d.constrained).sum() == 0
    torch.cuda.synchronize()  # no device-side assert was raised


def test_a_model_with_a_semantic_mask_is_refused(dev):
    g = bar_model(dev, P=64, optimizer=None)
    g._semantics_masks = torch.ones(16, device=dev)
    with pytest.raises(ValueError, match="semantic mask"):
        deform.Deformation(g, spacing=0.2)


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------
def test_a_bar_with_one_end_pinned_and_the_other_turned(dev):
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera, make_scene
    P = 2000
    sc = make_scene(P, S=16, seed=5, log_scale_mean=-3.0)
    tt = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).contiguous()  # noqa: E731
    g = dref.Model()
    g._xyz = nn.Parameter(tt(cases.bar(P, 9, length=2.0, width=0.25) - np.float32([1.0, 0.0, 0.0])))
    g._scaling = nn.Parameter(tt(np.log(sc.scales)))
    g._rotation = nn.Parameter(tt(sc.rotations))
    g._opacity = nn.Parameter(tt(np.log(sc.opacities / (1 - sc.opacities))))
    g._features_dc = nn.Parameter(tt(sc.shs[:, :1]))
    g._features_rest = nn.Parameter(tt(sc.shs[:, 1:]))
    g._semantics = nn.Parameter(tt(sc.semantics))
    assert g._features_rest.shape[1] == 15 and g._semantics.shape[1] == 16
    before = {attr: host(getattr(g, attr)) for _, attr in dref.PARAMS}
    d = deform.Deformation(g, spacing=0.2)
    pinned, handle = d.x[:, 0] < -0.6, d.x[:, 0] > 0.6
    quarter = cases.axis_angle((1, 0, 0), 90.0)
    d.constrain(pinned, d.x[pinned]).drag(handle, rotation=quarter, pivot=(1.0, 0.0, 0.0))
    x, idx, con, target = host(d.x), host(d.idx), host(d.constrained), host(d.target)
    naive_y = np.where(con[:, None].astype(bool), target, x)
    ident = np.tile(np.float32([1, 0, 0, 0]), (d.M, 1))
    E_naive = float(deform.energy(d.x, d.idx, t(naive_y, dev), t(ident, dev)))
    d.solve(iterations=50).apply()
    E = float(d.energy())
    y64, q64 = ref.solve(x, idx, None, con, target, iterations=50, dtype=np.float64)
    y32, q32 = ref.solve(x, idx, None, con, target, iterations=50, dtype=np.float32)
    E64, E32, En64 = ref.energy(x, idx, None, y64, q64), ref.energy(x, idx, None, y32, q32), ref.energy(x, idx, None, naive_y, ident)
    factor = E64 / En64
    tol = energy_tol(E64, E32)
    print(f"bar: {d.M} nodes, naive E {E_naive:.6e} (reference {En64:.6e}), solved E {E:.6e} (reference {E64:.6e}, twin {E32:.6e}), "
          f"factor {factor:.4f}, tol {tol:.3e}")
    assert abs(E_naive - En64) <= 1e-9 * En64
    assert factor < 0.2                      # what the CPU reference reaches on this case
    assert abs(E - E64) <= tol and E <= factor * E_naive + tol
    y = host(d.y)
    assert same_bits(y[con.astype(bool)], target[con.astype(bool)])
    after = {attr: host(getattr(g, attr)) for _, attr in dref.PARAMS}
    for attr in before:
        assert same_bits(after[attr], before[attr]) != (attr in ("_xyz", "_rotation", "_features_rest")), attr
    # the handle's Gaussians turned with it: far from the pinned end every Gaussian is near the rigid image of its rest position
    far = before["_xyz"][:, 0] > 0.8
    R = cases.quat_matrix(quarter)
    rigid = (before["_xyz"][far].astype(np.float64) - [1.0, 0, 0]) @ R.T + [1.0, 0, 0]
    assert np.abs(after["_xyz"][far] - rigid).max() < 0.05
    with torch.no_grad():
        out = render(TorchCamera(make_camera(96, 64, yaw=0.3, pitch=-0.2), dev), g, PipelineParams(), torch.tensor([0.1, 0.2, 0.3], device=dev))
    for k in ("render", "semantics", "depth", "alpha"):
        assert bool(torch.isfinite(out[k]).all()), k
    assert float(out["alpha"].min()) >= 0.0 and float(out["alpha"].max()) <= 1.0
    assert float(out["alpha"].max()) > 0.0   # the bar is in the picture
