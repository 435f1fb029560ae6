"""Every backward mode through the reference model's activations.

The other GPU tests of the autograd surface render render.GaussianSet, whose parameters ARE the rasterizer's operands.  The model
this package trains hands the rasterizer exp(_scaling), sigmoid(_opacity), normalize(_rotation), cat(_features_dc,
_features_rest), _semantics * mask and, under a Gaussian mask, t[mask]: non-leaf tensors with autograd nodes between them and the
parameters (tests/activated_model.py).  The reference of every test here is the composition
    chain(model, gradients of twin(model))
of the operand-leaf path -- held against the oracle and float64 elsewhere -- with torch's own activation backward: the same
kernels see the same operands, torch's nodes see the same gradients, so the assertions are torch.equal.  One test anchors the
whole composition in float64, independently of `chain`.

Scenes: 4000 Gaussians in a box wider than the frustum (extent (6, 4, 1)), S = 16, degree 3, 160 x 104, three cameras by yaw --
38 to 49 % of the Gaussians are culled per view, 62 % in some view, 16 % (626) in all three; and the parity suite's S = 3 case (1500
Gaussians, degree 1, 96 x 80) for the float64 anchor."""
import numpy as np
import pytest
import torch

from tests import activated_model as am

pytestmark = pytest.mark.gpu
W, H, S, DEG = 160, 104, 16, 3
MAIN = dict(P=4000, S=S, sh_degree=DEG, seed=17, extent=(6.0, 4.0, 1.0), log_scale_mean=-3.0)
YAWS, FOVX = (-0.4, 0.0, 0.4), 1.3
KEYS = ("render", "semantics", "depth", "alpha")
# the op's result (dL_dmeans2D, dL_dcolors, dL_dsemantics, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
STATE_TO_OPERAND = {"xyz": 4, "features": 6, "semantics": 2, "opacity": 3, "scaling": 7, "rotation": 8}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext(dev):
    from goi_hyperplane_amd import _C
    e = _C._ext()
    assert e is not None, "the compiled binding is not built (the gradient pool and the accumulating backward live there)"
    return e


class _Scene:
    def __init__(self, dev, W, H, cams, up_seed, **make_kwargs):
        from goi_hyperplane_amd.render import PipelineParams, TorchCamera
        S = make_kwargs["S"]
        self.dev, self.W, self.H, self.S = dev, W, H, S
        self.model = am.make(dev, **make_kwargs)
        self.P = self.model._xyz.shape[0]
        self.np_cams = cams
        self.cams = [TorchCamera(c, dev) for c in cams]
        # seeded upstream gradients on render, semantics, depth and alpha, per view (numpy: the float64 reference reads them too)
        g = np.random.default_rng(up_seed)
        self.np_ups = [[(g.standard_normal(shape) / (W * H)).astype(np.float32) for shape in ((3, H, W), (S, H, W), (1, H, W), (1, H, W))]
                       for _ in cams]
        self.ups = [[torch.tensor(u, device=dev) for u in up] for up in self.np_ups]
        self.bg = torch.zeros(3, device=dev)
        self.pipe = PipelineParams()


@pytest.fixture(scope="module")
def main(dev):
    from goi_hyperplane_amd.scene import make_camera
    return _Scene(dev, W, H, [make_camera(W, H, fovx=FOVX, yaw=y) for y in YAWS], 23, **MAIN)


def _clear(pc):
    for p in (pc.parameters() if hasattr(pc, "parameters") else am.raw_parameters(pc, trainable_only=False).values()):
        p.grad = None


def _backward(sc, pc, k, pipe=None, keys=KEYS, **render_kwargs):
    """one render of view k and its backward under the view's upstream gradients; -> (render()'s dictionary, backward kernel)"""
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.render import render
    out = render(sc.cams[k], pc, pipe or sc.pipe, sc.bg, **render_kwargs)
    torch.autograd.backward([out[key] for key in keys], [sc.ups[k][KEYS.index(key)] for key in keys])
    return out, rasterizer.last_backward_kernel()


def _raw_grads(model):
    """{raw attribute: clone of its .grad, or None}; the gradients are dropped (a pooled buffer goes back to the pool)"""
    out = {}
    for a, p in am.raw_parameters(model, trainable_only=False).items():
        out[a] = None if p.grad is None else p.grad.detach().clone()
        p.grad = None
    return out


def _assert_same(got, want, what):
    for a in am.RAW:
        assert (got[a] is None) == (want[a] is None), (what, a)
        if want[a] is not None:
            assert got[a].shape == want[a].shape and torch.equal(got[a], want[a]), (
                what, a, float((got[a].double() - want[a].double()).abs().max()), float(want[a].abs().max()))


def _model_and_twin(sc, k, pipe=None, raw_rotation=False, **render_kwargs):
    """the activated model's raw gradients of view k, and chain() of its twin's operand gradients in the same mode;
    -> dict(raw, chained, kernel, twin_kernel, out, twin_out, twin)"""
    model = sc.model
    _clear(model)
    out, kernel = _backward(sc, model, k, pipe, **render_kwargs)
    raw = _raw_grads(model)
    pc = am.twin(model, raw_rotation)
    twin_out, twin_kernel = _backward(sc, pc, k, pipe, **render_kwargs)
    chained = am.chain(model, am.twin_gradients(pc), raw_rotation)
    return dict(raw=raw, chained=chained, kernel=kernel, twin_kernel=twin_kernel, out=out, twin_out=twin_out, twin=pc)


@pytest.fixture(scope="module")
def plain(main, ext):
    """the plain full backward of the three views, pool off: {view: raw gradients}, and the radii; left unchanged by every test"""
    ext.set_grad_pool(False)
    try:
        res = []
        for k in range(3):
            _clear(main.model)
            out, kernel = _backward(main, main.model, k)
            assert kernel == "full"
            res.append(dict(raw=_raw_grads(main.model), radii=out["radii"].clone(), vs=out["viewspace_points"].grad.clone()))
    finally:
        ext.set_grad_pool(True)
    return res


def test_the_main_scene_culls(main, plain):
    culled = torch.stack([r["radii"] == 0 for r in plain])
    shares = [float(c.float().mean()) for c in culled]
    some, every = float(culled.any(0).float().mean()), float(culled.all(0).float().mean())
    print(f"\nactivated-model main scene: culled per view {shares}, in some view {some:.4f}, in all views {every:.4f}")
    assert all(0.2 <= s <= 0.8 for s in shares), shares
    assert 0.2 <= some <= 0.8, some
    assert every * main.P > 400, every  # rows no view sees: what the zero-row assertions below look at


# ---- (a) plain full backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [False, True])
def test_plain_backward_equals_the_chained_twin(main, plain, ext, pool):
    """cam0, cam1, cam2, cam0, cam1, cam2: with the pool on, model and twin take turns on the pooled buffers, reused with the rows
    of Gaussians invisible then and now skipped -- an autograd node (exp, sigmoid, normalize, cat) consumes the pooled views
    where the leaf case stores them in .grad"""
    ext.set_grad_pool(pool)
    try:
        h0 = ext.grad_pool_stats()
        for k in (0, 1, 2, 0, 1, 2):
            r = _model_and_twin(main, k)
            assert r["kernel"] == "full" and r["twin_kernel"] == "full"
            _assert_same(r["raw"], r["chained"], ("chain", pool, k))
            _assert_same(r["raw"], plain[k]["raw"], ("pool-less", pool, k))
            assert all(r["raw"][a] is not None for a in am.RAW)
            assert torch.equal(r["out"]["viewspace_points"].grad, r["twin_out"]["viewspace_points"].grad), (pool, k)
            assert torch.equal(r["out"]["viewspace_points"].grad, plain[k]["vs"]), (pool, k)
            for key in KEYS + ("radii",):
                assert torch.equal(r["out"][key], r["twin_out"][key]), (pool, k, key)
            del r  # (the twin's leaves hold views of a pooled buffer)
        if pool:
            assert ext.grad_pool_stats()[0] - h0[0] >= 6, (h0, ext.grad_pool_stats())  # hits: reused with rows skipped
    finally:
        ext.set_grad_pool(True)


# ---- (b) float64 anchor, independent of chain -------------------------------------------------------------------------------
def test_raw_gradients_against_float64_through_float64_activations(dev):
    """The S = 3 scene (1500 Gaussians, degree 1, 96 x 80, log-scale mean -2.5, rotation norms 0.5 .. 2) against
    tests/torch_reference.render in float64 behind float64 activations; gate: the suite's BWD_TOL (1e-3 of each tensor's scale).
    The same reference in float32 on the CPU stays within BWD_TOL / 10 of the float64 one on this scene (docs/MEASUREMENT_LOG.md:
    at most 1.1e-5, on _rotation), so the yardstick alone cannot fail the gate."""
    from goi_hyperplane_amd.scene import make_camera
    from tests.test_gpu_parity import BWD_TOL, check_backward
    from tests.torch_reference import float64_raw_gradients
    w, h = 96, 80
    sc = _Scene(dev, w, h, [make_camera(w, h, yaw=0.2)], 5, P=1500, S=3, sh_degree=1, seed=21, log_scale_mean=-2.5)
    raw = {a: p.detach().cpu().numpy() for a, p in am.raw_parameters(sc.model).items()}
    want = float64_raw_gradients(raw, sc.np_cams[0], np.zeros(3, np.float32), sc.np_ups[0], 1)
    _out, kernel = _backward(sc, sc.model, 0)
    assert kernel == "full"
    got = {a: g.cpu().numpy() for a, g in _raw_grads(sc.model).items()}
    for a in am.RAW:
        scale = float(np.abs(want[a]).max())
        print(f"\nactivated-model float64 anchor: {a} scale {scale:.3e} GPU err / scale {float(np.abs(got[a] - want[a]).max()) / scale:.3e}")
    check_backward(got, want, "activated_model_float64", tol=BWD_TOL, names=am.RAW)


# ---- (c) mode selection and results for non-leaf operands -------------------------------------------------------------------
def test_semantic_stage_with_a_mask(main, plain):
    from goi_hyperplane_amd import rasterizer
    model = main.model
    mask = (torch.rand(main.P, device=main.dev, generator=torch.Generator(device=main.dev).manual_seed(4)) < 2.0 / 3.0).float()
    assert 0.25 < 1.0 - float(mask.mean()) < 0.42
    try:
        am.set_trainable(model, "_semantics")
        model.set_semantic_masks(mask)
        r = _model_and_twin(main, 1)
        assert r["kernel"] == "semantics" and r["twin_kernel"] == "semantics"
        assert rasterizer.last_backward_kernel() == "semantics"
        _assert_same(r["raw"], r["chained"], "semantic stage")
        g = r["raw"]["_semantics"]
        assert all(r["raw"][a] is None for a in am.RAW if a != "_semantics")
        assert float(g.abs().max()) > 0 and float(g[mask == 0].abs().max()) == 0.0
        assert torch.equal(g, mask[:, None] * r["twin"]._semantics.grad)
        assert bool((r["twin"]._semantics.grad[mask == 0] != 0).any())  # (the twin's rows there are not zero: the mask did it)
    finally:
        model.set_semantic_masks(None)
        am.set_trainable(model)


def test_frozen_sh_takes_the_backward_without_the_sh_row(main, plain):
    try:
        am.set_trainable(main.model, *(a for a in am.RAW if "features" not in a))
        r = _model_and_twin(main, 2)
        assert r["kernel"] == "full_no_dsh" and r["twin_kernel"] == "full_no_dsh"
        _assert_same(r["raw"], r["chained"], "frozen SH")
        assert r["raw"]["_features_dc"] is None and r["raw"]["_features_rest"] is None
        for a in am.RAW:  # dropping the dL/dSH row changes nothing else
            if "features" not in a:
                assert torch.equal(r["raw"][a], plain[2]["raw"][a]), a
    finally:
        am.set_trainable(main.model)


def test_partial_gating_xyz_and_opacity(main, plain):
    try:
        am.set_trainable(main.model, "_xyz", "_opacity")
        r = _model_and_twin(main, 0)
        assert r["kernel"] == r["twin_kernel"] == "full_no_dsh"
        _assert_same(r["raw"], r["chained"], "partial gating")
        assert sorted(a for a in am.RAW if r["raw"][a] is not None) == ["_opacity", "_xyz"]
        for a in ("_xyz", "_opacity"):
            assert torch.equal(r["raw"][a], plain[0]["raw"][a]), a
    finally:
        am.set_trainable(main.model)


def test_sh_factored_leaves_the_sh_leaves_to_the_factor(main, plain):
    from goi_hyperplane_amd import _C, rasterizer
    model = main.model
    rasterizer.set_backward_mode(sh_factored=True)
    try:
        _clear(model)
        _out, kernel = _backward(main, model, 1)
        factor = rasterizer.take_sh_factor()
        raw = _raw_grads(model)
        pc = am.twin(model)
        _tout, twin_kernel = _backward(main, pc, 1)
        twin_factor = rasterizer.take_sh_factor()
        chained = am.chain(model, am.twin_gradients(pc))
    finally:
        rasterizer.set_backward_mode(sh_factored=False)
    assert kernel == "factored" and twin_kernel == "factored"
    assert raw["_features_dc"] is None and raw["_features_rest"] is None and pc._features.grad is None
    _assert_same(raw, chained, "sh_factored")
    for a in am.RAW:
        if "features" not in a:
            assert torch.equal(raw[a], plain[1]["raw"][a]), a
    assert factor is not None and torch.equal(factor["gcol"], twin_factor["gcol"])
    M = (DEG + 1) ** 2
    dsh = _C.sh_grad_from_views(model.get_xyz.detach(), factor["campos"].reshape(1, 3), factor["gcol"][None].contiguous(), DEG, M)
    assert torch.equal(dsh[:, :1], plain[1]["raw"]["_features_dc"])
    assert torch.equal(dsh[:, 1:], plain[1]["raw"]["_features_rest"])


# ---- (d) Python-side operand paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["compute_cov3D_python", "convert_SHs_python"])
def test_python_side_operand_paths(main, flag):
    """the chain to _scaling / _rotation (covariance) or to _features_* and _xyz (colours) runs in torch instead of in the kernel;
    the twin of the covariance path holds the RAW quaternions: get_covariance reads _rotation, not get_rotation"""
    from goi_hyperplane_amd.render import PipelineParams
    cov = flag == "compute_cov3D_python"
    r = _model_and_twin(main, 0, pipe=PipelineParams(**{flag: True}), raw_rotation=cov)
    assert r["kernel"] == "full" and r["twin_kernel"] == "full"
    _assert_same(r["raw"], r["chained"], flag)
    assert all(r["raw"][a] is not None and float(r["raw"][a].abs().max()) > 0 for a in am.RAW), flag
    assert torch.equal(r["out"]["viewspace_points"].grad, r["twin_out"]["viewspace_points"].grad)


@pytest.mark.parametrize("in_place", [False, True])
def test_gaussian_mask_selects_activations(main, in_place):
    m = torch.rand(main.P, device=main.dev, generator=torch.Generator(device=main.dev).manual_seed(6)) < 0.5
    assert 0.45 < float(m.float().mean()) < 0.55
    r = _model_and_twin(main, 2, gaussian_mask=m, in_place=in_place)
    assert r["kernel"] == "full" and r["twin_kernel"] == "full"
    _assert_same(r["raw"], r["chained"], ("gaussian_mask", in_place))
    for a in am.RAW:
        g = r["raw"][a]
        assert float(g[m].abs().max()) > 0 and float(g[~m].abs().max()) == 0.0, (a, in_place)
    vs = r["out"]["viewspace_points"].grad
    assert torch.equal(vs, r["twin_out"]["viewspace_points"].grad) and float(vs[~m].abs().max()) == 0.0


# ---- (e), (f) multi-view batches --------------------------------------------------------------------------------------------
def _render_view(sc):
    from goi_hyperplane_amd.render import render
    return lambda cam: render(cam, sc.model, sc.pipe, sc.bg)


def _upstream(sc):
    return lambda o, k: ((o["render"], o["semantics"]), tuple(sc.ups[k][:2]))


def _params(model):
    return list(am.raw_parameters(model).values())


@pytest.fixture(scope="module")
def serial(main, plain, ext):
    """K backward() calls on the activated model, render and semantics upstream: p.grad after two and after three views, and
    every view's viewspace_points.grad"""
    from goi_hyperplane_amd.render import render
    model = main.model
    _clear(model)
    res = dict(vs=[], after={})
    for k in range(3):
        out = render(main.cams[k], model, main.pipe, main.bg)
        torch.autograd.backward((out["render"], out["semantics"]), tuple(main.ups[k][:2]))
        res["vs"].append(out["viewspace_points"].grad.clone())
        res["after"][k + 1] = {a: p.grad.clone() for a, p in am.raw_parameters(model).items()}
    _clear(model)
    return res


def _grads_now(model):
    return {a: (None if p.grad is None else p.grad.clone()) for a, p in am.raw_parameters(model, trainable_only=False).items()}


def _plain_is_still_exact(main, plain):
    _clear(main.model)
    _out, kernel = _backward(main, main.model, 0)
    assert kernel == "full"
    _assert_same(_raw_grads(main.model), plain[0]["raw"], "a plain backward after the batches")


@pytest.mark.parametrize("K,streams", [(3, 1), (2, 2)])
def test_batch_of_leaf_sums_equals_the_serial_backward(main, plain, serial, K, streams):
    """on_device=False: K dense sums of leaf gradients, (g0 + g1) + g2 on one stream and g0 + g1 on two: what K backward() calls
    leave in p.grad, bit for bit; every returned viewspace_points carries the serial view's gradient"""
    from goi_hyperplane_amd import dist, rasterizer
    model = main.model
    for rep in range(2):  # (twice: the second batch reuses pooled buffers and scratch)
        _clear(model)
        outs = dist.backward_views(main.cams[:K], _render_view(main), _upstream(main), _params(model), streams=streams, on_device=False)
        torch.cuda.synchronize()
        assert rasterizer.last_backward_kernel() == "full"
        _assert_same(_grads_now(model), serial["after"][K], (rep, K, streams))
        for k in range(K):
            assert torch.equal(outs[k]["viewspace_points"].grad, serial["vs"][k]), (rep, k)
    _plain_is_still_exact(main, plain)


def _by_hand(main):
    """the protocol by hand: accumulate_gradients(state) around each render + autograd.grad, then dist.accumulated_gradients"""
    from goi_hyperplane_amd import dist, rasterizer
    from goi_hyperplane_amd.render import render
    model = main.model
    params = am.raw_parameters(model)
    state = dict(grads=None, inputs=None, views=0)
    sinks = []
    for k in range(3):
        with rasterizer.accumulate_gradients(state):
            out = render(main.cams[k], model, main.pipe, main.bg)
            g = torch.autograd.grad((out["render"], out["semantics"]), list(params.values()), tuple(main.ups[k][:2]),
                                    allow_unused=True, retain_graph=True)
        assert rasterizer.last_backward_kernel() == "full_accumulate" and all(t is None for t in g)
        sinks.append(out["viewspace_points"])
    got = dict.fromkeys(am.RAW)
    got.update(zip(params, dist.accumulated_gradients(state, list(params.values()))))
    return state, got, sinks


def test_accumulated_batch_by_hand(main, plain, serial):
    """state["grads"] against the serial sum of the twin's operand gradients (the bound tests/test_gpu_dist.py applies to the same
    sum: the association of fp32 additions differs), the helper against chain() of the same sums, and the rows no view sees"""
    model = main.model
    state, got, sinks = _by_hand(main)
    torch.cuda.synchronize()
    assert state["views"] == 3
    assert all(s.grad is None for s in sinks)
    chained = am.chain(model, {name: state["grads"][j] for name, j in STATE_TO_OPERAND.items()})
    _assert_same(got, chained, "helper against chain")
    pc = am.twin(model)
    for k in range(3):  # the twin's leaves sum their operand gradients serially
        _backward(main, pc, k, keys=KEYS[:2])
    for name, j in STATE_TO_OPERAND.items():
        want = am.twin_gradients(pc)[name]
        scale = float(want.abs().max())
        err = float((state["grads"][j].view_as(want) - want).abs().max())
        print(f"\naccumulated operand sum {name}: err {err:.3e} scale {scale:.3e}")
        assert err <= 4e-6 * scale + 1e-12, name
    unseen = torch.stack([r["radii"] == 0 for r in plain]).all(0)
    assert int(unseen.sum()) > 400
    for a in ("_scaling", "_opacity", "_rotation", "_features_dc", "_features_rest"):
        assert float(got[a][unseen].abs().max()) == 0.0 and float(got[a][~unseen].abs().max()) > 0, a
    _plain_is_still_exact(main, plain)


def test_batch_summed_on_the_device(main, plain, serial):
    """on_device=True (the default): does not raise behind activations, takes the accumulating backward, and p.grad is the
    hand-run protocol's result bit for bit -- on one stream and on two (the event chain keeps the accumulation in view order);
    an extra loss term that bypasses the rasterizer arrives exactly once; accumulate=True adds to what is there; no returned
    viewspace_points has a gradient"""
    from goi_hyperplane_amd import dist, rasterizer
    model = main.model
    _state, hand, _sinks = _by_hand(main)
    hand = {a: (None if g is None else g.clone()) for a, g in hand.items()}
    del _state, _sinks
    for streams in (1, 2):
        for rep in range(2):
            _clear(model)
            outs = dist.backward_views(main.cams, _render_view(main), _upstream(main), _params(model), streams=streams)
            torch.cuda.synchronize()
            assert rasterizer.last_backward_kernel() == "full_accumulate"
            _assert_same(_grads_now(model), hand, (streams, rep))
            assert len(outs) == 3 and all(o["viewspace_points"].grad is None for o in outs)
            for k in range(3):
                assert torch.equal(outs[k]["radii"], plain[k]["radii"])
    _plain_is_still_exact(main, plain)
    # the extra term: 1e-3 * mean(get_scaling) on view 0's loss
    extra = torch.autograd.grad(1e-3 * model.get_scaling.mean(), model._scaling)[0]

    def upstream(o, k):
        if k == 0:
            return (o["render"], o["semantics"], 1e-3 * model.get_scaling.mean()), tuple(main.ups[k][:2]) + (torch.ones((), device=main.dev),)
        return (o["render"], o["semantics"]), tuple(main.ups[k][:2])
    want = dict(hand, _scaling=hand["_scaling"] + extra)
    _clear(model)
    dist.backward_views(main.cams, _render_view(main), upstream, _params(model), streams=1)
    _assert_same(_grads_now(model), want, "extra term, on the device")
    # accumulate=True
    gen = torch.Generator(device=main.dev).manual_seed(9)
    held = {a: torch.randn(p.shape, device=main.dev, generator=gen) * 1e-3 for a, p in am.raw_parameters(model).items()}
    for a, p in am.raw_parameters(model).items():
        p.grad = held[a].clone()
    dist.backward_views(main.cams, _render_view(main), _upstream(main), _params(model), streams=1, accumulate=True)
    _assert_same(_grads_now(model), {a: held[a] + hand[a] for a in am.RAW}, "accumulate=True")
    _clear(model)


def test_extra_loss_term_arrives_once_in_the_leaf_sums(main, serial):
    from goi_hyperplane_amd import dist
    from goi_hyperplane_amd.render import render
    model = main.model
    _clear(model)
    for k in range(3):  # the serial reference with the term on view 0
        out = render(main.cams[k], model, main.pipe, main.bg)
        loss = (out["render"] * main.ups[k][0]).sum() + (out["semantics"] * main.ups[k][1]).sum()
        (loss + 1e-3 * model.get_scaling.mean() if k == 0 else loss).backward()
    want = _raw_grads(model)
    extra = torch.autograd.grad(1e-3 * model.get_scaling.mean(), model._scaling)[0]
    bound = 4e-6 * float(want["_scaling"].abs().max()) + 1e-12  # (against the term-less serial sum: another association)
    assert float((want["_scaling"] - extra - serial["after"][3]["_scaling"]).abs().max()) <= bound

    def upstream(o, k):
        loss = (o["render"] * main.ups[k][0]).sum() + (o["semantics"] * main.ups[k][1]).sum()
        return (loss + 1e-3 * model.get_scaling.mean() if k == 0 else loss,), (torch.ones((), device=main.dev),)
    dist.backward_views(main.cams, _render_view(main), upstream, _params(model), streams=1, on_device=False)
    _assert_same(_grads_now(model), want, "extra term, leaf sums")
    _clear(model)


def test_render_views_on_side_streams_equal_the_serial_loop(main):
    from goi_hyperplane_amd.render import render, render_views
    model = main.model
    loss = lambda i, o: (o["render"] * main.ups[i][0]).sum() + (o["semantics"] * main.ups[i][1]).sum()  # noqa: E731
    _clear(model)
    ref = []
    for i, cam in enumerate(main.cams):
        o = render(cam, model, main.pipe, main.bg)
        loss(i, o).backward()
        ref.append({k: o[k].detach().clone() for k in KEYS + ("radii",)} | {"vs": o["viewspace_points"].grad.clone()})
    want = _raw_grads(model)
    outs = render_views(main.cams, model, main.pipe, main.bg, loss_fn=loss, streams=2)
    torch.cuda.synchronize()
    _assert_same(_raw_grads(model), want, "render_views")
    for i in range(3):
        for k in KEYS + ("radii",):
            assert torch.equal(outs[i][k].detach(), ref[i][k]), (i, k)
        assert torch.equal(outs[i]["viewspace_points"].grad, ref[i]["vs"]), i
