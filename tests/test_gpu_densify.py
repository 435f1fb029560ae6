"""goi_hyperplane_amd.densify (csrc/densify.hip) on the GPU: against the reference's own methods (the CPU pins of
tests/golden/ref_densify_pins.npz, recorded normal draws replayed), and against the densification semantics of
tests/densify_reference.py run on the same device: sizes from 0 to 1 M, every edge of the decisions (nothing selected,
everything cloned / split / pruned, max_screen_size, thresholds at the rounded value and 1 ulp either side), optimizer None,
partial groups, state never stepped, torch.optim.Adam and FusedAdam, the same seed giving the same children; the statistics
without host synchronisation; GOI's 3D delete and extract against the rasterizer's gaussian_mask; and a densifying
training loop."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import densify_reference as ref

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float32).eps)
ARGS = dict(max_grad=2e-4, min_opacity=0.1, extent=4.0)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def assert_bits(a, b, what):
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    if not torch.equal(bits(a), bits(b)):
        d = (a.detach().double() - b.detach().double()).abs()
        raise AssertionError(f"{what}: {int((bits(a) != bits(b)).sum())} elements differ, max {float(d.max())}")


def assert_children(a, b, first, s_norm, what):
    """rows before the children bit-exact; children's xyz within 4 ulp of max(|xyz|, |sample|) (bmm against an FMA chain),
    log-scales within 2 ulp of max(|v|, 1)"""
    assert_bits(a[:first], b[:first], what)
    ca, cb = a[first:].detach().double(), b[first:].detach().double()
    if what == "_xyz":
        tol = 4 * EPS * torch.maximum(cb.abs(), s_norm.double().to(cb.device)[:, None])
    else:
        tol = 2 * EPS * torch.clamp(cb.abs(), min=1.0)
    assert not bool(((ca - cb).abs() > tol).any()), (what, float((ca - cb).abs().max()))


def check_optimizer(hip, rst):
    if rst.optimizer is None:
        assert hip.optimizer is None
        return
    assert [g["name"] for g in hip.optimizer.param_groups] == [g["name"] for g in rst.optimizer.param_groups]
    for gh, gr in zip(hip.optimizer.param_groups, rst.optimizer.param_groups):
        p = gh["params"][0]
        assert p is getattr(hip, ref.ATTR[gh["name"]]) and isinstance(p, nn.Parameter) and p.requires_grad
        sh, sr = hip.optimizer.state.get(p), rst.optimizer.state.get(gr["params"][0])
        assert (sh is None) == (sr is None), gh["name"]
        if sr:
            assert_bits(sh["exp_avg"], sr["exp_avg"], gh["name"] + " exp_avg")
            assert_bits(sh["exp_avg_sq"], sr["exp_avg_sq"], gh["name"] + " exp_avg_sq")
            assert float(sh["step"]) == float(sr["step"])
    assert len(hip.optimizer.state) == len(rst.optimizer.state)


def compare(hip, rst, info):
    first = info["kept"] + info["clones"]
    assert hip._xyz.shape[0] == first + 2 * info["children"] == rst._xyz.shape[0], (hip._xyz.shape, rst._xyz.shape, info)
    for _, attr in ref.PARAMS:
        a, b = getattr(hip, attr), getattr(rst, attr)
        assert isinstance(a, nn.Parameter) and a.requires_grad == b.requires_grad, attr
        if attr in ("_xyz", "_scaling"):
            assert_children(a, b, first, info["samples_norm"], attr)
        else:
            assert_bits(a, b, attr)
    for name in ref.STATS:
        assert_bits(getattr(hip, name), getattr(rst, name), name)
    check_optimizer(hip, rst)


def run_both(dev, P, seed=0, optimizer="adam", steps=2, percent_dense=0.01, max_screen_size=None, gen_seed=7,
             denom_zero=0.05, **kw):
    args = dict(ARGS, **kw)
    from goi_hyperplane_amd import densify
    hip = ref.make_model(P, dev, seed=seed, optimizer=optimizer, steps=steps, denom_zero=denom_zero)
    rst = ref.make_model(P, dev, seed=seed, optimizer=optimizer, steps=steps, denom_zero=denom_zero)
    hip.percent_dense = rst.percent_dense = percent_dense
    densify.densify_and_prune(hip, args["max_grad"], args["min_opacity"], args["extent"], max_screen_size,
                              generator=torch.Generator(device=dev).manual_seed(gen_seed))
    info = ref.densify_and_prune(rst, args["max_grad"], args["min_opacity"], args["extent"], max_screen_size,
                                 generator=torch.Generator(device=dev).manual_seed(gen_seed))
    compare(hip, rst, info)
    return hip, info


def _pinned_case(d, case, max_screen_size):
    """block sizes and the samples' norms of a pinned case, from the restatement on the CPU with the recorded draws
    (tests/test_densify_cpu.py holds that restatement bit-exact to these pins)"""
    z = torch.from_numpy(d[f"{case}_z"].copy())
    return ref.densify_and_prune(ref.pins_model(d, "cpu"), float(d["max_grad"]), float(d["min_opacity"]),
                                 float(d["extent"]), max_screen_size, normal=lambda mean, std: z * std + mean)


def _assert_pinned(m, d, case, info=None):
    """the model against the reference's pinned outputs: counts and order exact, copied rows and moments bit-exact;
    children's xyz within 4 ulp of max(|xyz|, |sample|), children's log-scales within 2 ulp of max(|v|, 1)"""
    got, want = ref.model_outputs(m), ref.pinned_outputs(d, case)
    first = None if info is None else info["kept"] + info["clones"]
    for k, w in want.items():
        g = torch.as_tensor(np.asarray(got[k], np.float32))
        w = torch.as_tensor(np.asarray(w, np.float32))
        if first is not None and k in ("_xyz", "_scaling"):
            assert_children(g, w, first, info["samples_norm"], k)
        else:
            assert_bits(g, w, f"{case}: {k}")
    check_rekeyed(m)


def check_rekeyed(m):
    for name, attr in ref.PARAMS:
        group = next(g for g in m.optimizer.param_groups if g["name"] == name)
        assert group["params"][0] is getattr(m, attr) and isinstance(getattr(m, attr), nn.Parameter)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case,max_screen_size", [("dp_none", None), ("dp_screen", 20)])
def test_densify_and_prune_against_the_reference_pins(dev, monkeypatch, case, max_screen_size, fused):
    """The kernels against the reference's own clone -> split -> prune-parents -> prune sequence
    (tests/golden/ref_densify_pins.npz, recorded on the CPU) with the recorded standard-normal draws replayed."""
    from goi_hyperplane_amd import densify
    d = ref.pins()
    z = torch.from_numpy(d[f"{case}_z"].copy())

    def recorded(n_split, device, generator):
        assert z.shape == (2 * n_split, 3), (z.shape, n_split)
        return z.to(device)
    monkeypatch.setattr(densify, "_draw_z", recorded)
    m = ref.pins_model(d, dev, fused)
    densify.densify_and_prune(m, float(d["max_grad"]), float(d["min_opacity"]), float(d["extent"]), max_screen_size)
    info = _pinned_case(d, case, max_screen_size)
    assert info["children"] > 0 and info["clones"] > 0
    _assert_pinned(m, d, case, info)


def test_prune_points_and_reset_opacity_against_the_reference_pins(dev):
    from goi_hyperplane_amd import densify
    d = ref.pins()
    m = ref.pins_model(d, dev)
    densify.prune_points(m, torch.from_numpy(d["prune_mask"].copy()).to(dev))
    _assert_pinned(m, d, "prune")
    m = ref.pins_model(d, dev)
    densify.reset_opacity(m)  # torch's sigmoid and log on the device against the CPU's: within 2 ulp
    got, want = ref.model_outputs(m), ref.pinned_outputs(d, "reset")
    a, b = torch.as_tensor(got["_opacity"]).double(), torch.as_tensor(want["_opacity"]).double()
    assert bool(((a - b).abs() <= 2 * EPS * torch.clamp(b.abs(), min=1.0)).all())
    for k in want:
        if k != "_opacity":
            assert_bits(torch.as_tensor(np.asarray(got[k], np.float32)), torch.as_tensor(np.asarray(want[k], np.float32)), k)
    check_rekeyed(m)


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 4097, 100_000, 1_000_000])
def test_densify_and_prune_matches_the_restatement(dev, P):
    hip, info = run_both(dev, P, seed=P % 97)
    if P >= 4097:  # a real mix of all three outcomes
        assert info["clones"] > 0 and info["children"] > 0 and info["kept"] < P - info["children"]


@pytest.mark.parametrize("case", ["nothing", "all_clone", "all_split", "all_pruned", "screen_20", "screen_negative"])
def test_densify_and_prune_edges(dev, case):
    P = 4097
    kw = {"nothing": dict(max_grad=1e9, min_opacity=0.0, denom_zero=0.0),  # (x / 0 = inf passes any finite max_grad)
          "all_clone": dict(max_grad=0.0, min_opacity=0.0, percent_dense=1e6),
          "all_split": dict(max_grad=-1.0, min_opacity=0.0, percent_dense=0.0),
          "all_pruned": dict(min_opacity=2.0),
          "screen_20": dict(max_screen_size=20),
          "screen_negative": dict(max_screen_size=-1)}[case]
    hip, info = run_both(dev, P, seed=3, **kw)
    n = hip._xyz.shape[0]
    if case == "nothing":
        assert n == P and info["clones"] == info["children"] == 0
    elif case == "all_clone":
        assert n == 2 * P and info["clones"] == P
    elif case == "all_split":
        assert n == 2 * P and info["children"] == P and info["kept"] == 0
    elif case in ("all_pruned", "screen_negative"):
        assert n == 0
    else:
        assert 0 < n < P + info["clones"] + 2 * info["children"] + 1


def _extent_for(target, factor):
    """an extent whose Python product factor * extent rounds to the fp32 value `target`"""
    e = float(target) / factor
    for _ in range(200):
        got = np.float32(factor * e)
        if got == np.float32(target):
            return e
        e = float(np.nextafter(e, np.inf if got < np.float32(target) else -np.inf))
    raise AssertionError("no extent found")


@pytest.mark.parametrize("which", ["max_grad", "scale", "opacity", "world"])
@pytest.mark.parametrize("ulp", [-1, 0, 1])
def test_thresholds_at_the_rounded_value_and_one_ulp_either_side(dev, which, ulp):
    P = 4097
    m = ref.make_model(P, dev, seed=11)
    with torch.no_grad():
        grad = (m.xyz_gradient_accum / m.denom).nan_to_num(0.0).reshape(-1)
        smax = torch.exp(m._scaling).max(dim=1).values
        op = torch.sigmoid(m._opacity).reshape(-1)
    r = int(torch.nonzero(grad > 0)[123])  # (a Gaussian with a finite, non-zero gradient)

    def f32(v):
        v = np.float32(float(v))
        return float(v if ulp == 0 else np.nextafter(v, np.float32(np.inf if ulp > 0 else -np.inf)))
    kw = {}
    if which == "max_grad":
        kw["max_grad"] = f32(grad[r])
    elif which == "scale":
        kw.update(percent_dense=0.01, extent=_extent_for(f32(smax[r]), 0.01))
    elif which == "opacity":
        kw["min_opacity"] = f32(op[r])
    else:
        kw.update(max_screen_size=20, extent=_extent_for(f32(smax[r]), 0.1))
    run_both(dev, P, seed=11, **kw)


@pytest.mark.parametrize("optimizer,steps", [(None, 0), ("partial", 2), ("adam", 0), ("fused", 2), ("fused", 0)])
def test_optimizer_variants(dev, optimizer, steps):
    hip, _ = run_both(dev, 5000, seed=2, optimizer=optimizer, steps=steps)
    if optimizer is not None:
        sd = hip.optimizer.state_dict()
        from goi_hyperplane_amd.optim import FusedAdam
        for cls in (torch.optim.Adam, FusedAdam):  # either optimizer loads what the re-keyed one saves
            params = [{"params": [getattr(hip, ref.ATTR[g["name"]])], "lr": g["lr"], "name": g["name"]}
                      for g in hip.optimizer.param_groups]
            cls(params, lr=0.0, eps=1e-15).load_state_dict(sd)


def test_default_generator_gives_the_restatements_children(dev):
    from goi_hyperplane_amd import densify
    hip = ref.make_model(4097, dev, seed=4)
    rst = ref.make_model(4097, dev, seed=4)
    torch.cuda.manual_seed(1234)
    densify.densify_and_prune(hip, ARGS["max_grad"], ARGS["min_opacity"], ARGS["extent"], None)
    torch.cuda.manual_seed(1234)
    info = ref.densify_and_prune(rst, ARGS["max_grad"], ARGS["min_opacity"], ARGS["extent"], None)
    compare(hip, rst, info)
    assert info["children"] > 0


def test_prune_points_matches_the_restatement(dev):
    from goi_hyperplane_amd import densify
    for optimizer in ("adam", "partial", None):
        hip = ref.make_model(10000, dev, seed=6, optimizer=optimizer)
        rst = ref.make_model(10000, dev, seed=6, optimizer=optimizer)
        mask = torch.rand(10000, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.3
        densify.prune_points(hip, mask)
        ref.prune_points(rst, mask)
        for _, attr in ref.PARAMS:
            assert_bits(getattr(hip, attr), getattr(rst, attr), attr)
        for name in ref.STATS:  # values kept
            assert_bits(getattr(hip, name), getattr(rst, name), name)
        check_optimizer(hip, rst)
    hip = ref.make_model(100, dev, seed=6)
    densify.prune_points(hip, torch.ones(100, dtype=torch.bool, device=dev))
    assert hip._xyz.shape[0] == 0 and hip.optimizer.state[hip._xyz]["exp_avg"].shape == (0, 3)


def test_reset_opacity_matches_the_restatement(dev):
    from goi_hyperplane_amd import densify
    for optimizer in ("fused", "partial"):
        hip = ref.make_model(5000, dev, seed=8, optimizer=optimizer)
        rst = ref.make_model(5000, dev, seed=8, optimizer=optimizer)
        densify.reset_opacity(hip)
        ref.reset_opacity(rst)
        assert_bits(hip._opacity, rst._opacity, "_opacity")
        check_optimizer(hip, rst)


def test_refusals(dev):
    from goi_hyperplane_amd import densify
    m = ref.make_model(100, dev, seed=1)
    m.set_semantic_masks(torch.ones(100, device=dev))
    with pytest.raises(ValueError, match="semantic mask"):
        densify.prune_points(m, torch.zeros(100, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="semantic mask"):
        densify.densify_and_prune(m, 2e-4, 0.1, 4.0, None)
    m.set_semantic_masks(None)
    vp = torch.zeros(100, 3, device=dev, requires_grad=True)
    with pytest.raises(ValueError, match="accumulate"):
        densify.add_densification_stats(m, vp, torch.ones(100, dtype=torch.bool, device=dev))


def test_add_densification_stats_without_a_host_sync(dev):
    from goi_hyperplane_amd import densify
    P, iters = 50000, 6
    hip = ref.make_model(P, dev, seed=9, optimizer=None)
    rst = ref.make_model(P, dev, seed=9, optimizer=None)
    g = torch.Generator(device=dev).manual_seed(2)
    vps, filters = [], []
    for _ in range(iters):
        vp = torch.zeros(P, 3, device=dev, requires_grad=True)
        vp.grad = torch.randn(P, 3, device=dev, generator=g) * 1e-3
        vps.append(vp)
        filters.append(torch.rand(P, device=dev, generator=g) < 0.7)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for vp, f in zip(vps, filters):
            densify.add_densification_stats(hip, vp, f)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for vp, f in zip(vps, filters):
        ref.add_densification_stats(rst, vp, f)
    assert_bits(hip.denom, rst.denom, "denom")
    a, b = hip.xyz_gradient_accum.double(), rst.xyz_gradient_accum.double()
    assert bool(((a - b).abs() <= iters * EPS * b.abs()).all()), float((a - b).abs().max())


def _scene_model(dev, P=20000, seed=4):
    from tests import activated_model
    return activated_model.make(dev, P, S=16, seed=seed, rotation_norm=None, log_scale_mean=-3.0)


def test_goi_delete_and_extract_render_as_the_gaussian_mask(dev):
    """gui/main.py:515-523 (edit_delete) is prune_points with the semantic selection; the "seg" view (:1183-1185) keeps the
    selection alone.  Both must render bit-equal to the rasterizer's gaussian_mask on the unpruned model."""
    from goi_hyperplane_amd import densify
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera
    from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, select_gaussians, svm_score_fn
    torch.manual_seed(8)
    mlp = SemanticModel(dim_in=16, dim_out=300, num_layer=1, use_bias=True, device=dev)
    pos_code = torch.rand(300, device=dev) < 0.3
    u = torch.nn.functional.normalize(torch.randn(256, device=dev), dim=0)
    lut = torch.randn(300, 256, device=dev) * 0.1 + 0.2 * (2 * pos_code.float() - 1)[:, None] * u[None]
    svm = LinearSVM().to(dev)
    svm.weight_set(u.reshape(1, -1))
    cam = TorchCamera(make_camera(256, 192, yaw=0.2), dev)
    bg = torch.tensor([0.0, 0.1, 0.2], device=dev)
    base = _scene_model(dev)
    mask = select_gaussians(base, mlp, lut, svm_score_fn(svm))
    assert 0 < int(mask.sum()) < mask.numel()
    for keep_selection in (False, True):
        pruned = _scene_model(dev)
        densify.prune_points(pruned, ~mask if keep_selection else mask)
        with torch.no_grad():
            want = render(cam, base, PipelineParams(), bg, gaussian_mask=mask if keep_selection else ~mask)
            got = render(cam, pruned, PipelineParams(), bg)
        for k in ("render", "semantics", "depth", "alpha", "radii"):
            assert torch.equal(got[k], want[k]), (keep_selection, k)


def _train(dev, use_hip, iters=12, every=4):
    from goi_hyperplane_amd import densify, rasterizer
    from goi_hyperplane_amd.optim import FusedAdam
    from goi_hyperplane_amd.photometric import photometric_loss
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera
    m = _scene_model(dev, P=3000, seed=1)
    m.percent_dense = 0.01
    lrs = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "semantics": 1e-3, "opacity": 0.05, "scaling": 5e-3,
           "rotation": 1e-3}
    m.optimizer = FusedAdam([{"params": [getattr(m, ref.ATTR[n])], "lr": lr, "name": n} for n, lr in lrs.items()],
                            lr=0.0, eps=1e-15)
    cams = [TorchCamera(make_camera(96, 64, yaw=0.1 * i), dev) for i in range(3)]
    g = torch.Generator(device=dev).manual_seed(5)
    gts = [torch.rand(3, 64, 96, device=dev, generator=g) for _ in range(3)]
    bg = torch.zeros(3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    counts, overflows = [], []
    for it in range(iters):
        out = render(cams[it % 3], m, PipelineParams(), bg)
        loss, _ = photometric_loss(out["render"], gts[it % 3])
        loss.backward()
        with torch.no_grad():
            if use_hip:
                densify.add_densification_stats(m, out["viewspace_points"], out["visibility_filter"])
            else:
                ref.add_densification_stats(m, out["viewspace_points"], out["visibility_filter"])
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        if it % every == every - 1:
            before = rasterizer.speculation_stats()["overflows"]
            grad = (m.xyz_gradient_accum / m.denom).nan_to_num(0.0)
            max_grad = float(torch.quantile(grad[grad > 0], 0.7)) if use_hip else _train.max_grads[len(counts)]
            if use_hip:
                _train.max_grads.append(max_grad)
                densify.densify_and_prune(m, max_grad, 0.005, 8.0, None, generator=gen)
            else:
                ref.densify_and_prune(m, max_grad, 0.005, 8.0, None, generator=gen)
            counts.append(m._xyz.shape[0])
            out = render(cams[0], m, PipelineParams(), bg)  # a frame at the new P
            int(rasterizer.last_num_rendered())
            overflows.append(rasterizer.speculation_stats()["overflows"] - before)
    return m, counts, overflows


_train.max_grads = []


def test_densifying_training_loop_tracks_the_restatement(dev):
    _train.max_grads.clear()
    a, ca, oa = _train(dev, True)
    b, cb, ob = _train(dev, False)
    assert ca == cb and len(set(ca)) > 1, (ca, cb)
    assert oa == [0] * len(oa) and ob == [0] * len(ob), (oa, ob)
    iters = 12
    for name, attr in ref.PARAMS:
        x, y = getattr(a, attr).detach(), getattr(b, attr).detach()
        assert x.shape == y.shape
        lr = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "semantics": 1e-3, "opacity": 0.05, "scaling": 5e-3,
              "rotation": 1e-3}[name]
        d = (x - y).abs().flatten()
        assert float(torch.quantile(d[: 1 << 22].double(), 0.999)) <= 0.05 * lr * iters, name
        assert float(d.max()) <= 2 * lr * iters + 1e-5 * float(y.abs().max()), name
