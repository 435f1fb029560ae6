"""The forward's frame driver (_C._rasterize_gaussians_frame) under BOTH bindings: one scripted sequence of frames -- default
policy, forced overflow read and unread, selected frames, a truncation window, the geometry cache, a depth cut that holds and
one that fails -- is driven through render() once with the compiled binding and once with ctypes.  Only the launch differs
between the two, so everything else must agree: outputs and gradients bit for bit, what num_rendered is and says about its
frame, and every counter the frames move.  The compiled run is also held against exact-mode frames, so the two bindings cannot
agree on a wrong picture."""
import warnings

import pytest
import torch

from goi_hyperplane_amd.scene import make_camera, make_scene
from tests.test_gpu_depth_cut import _setup as depth_cut_setup

pytestmark = pytest.mark.gpu

OUTS = ("render", "semantics", "depth", "alpha", "radii")
P, S, W, H = 3000, 10, 160, 120  # 80 tiles, a partial tile row, S != 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _C
    _C.set_binding("compiled")  # fails loudly if lib/_goi_C.so has not been built
    return torch.device("cuda:0")


def _restore():
    from goi_hyperplane_amd import _C, rasterizer
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _C.poll_counts(wait=True)
    _C.set_binding("compiled")
    _C.set_forward_mode(speculative=True, headroom=2.0, capacity=None, on_overflow="warn", max_ahead=64,
                        inference_speculative=False, min_history=3, depth_cut=False)
    rasterizer.set_geometry_cache(0)
    rasterizer.accumulate_truncation(None)
    _C.forget_depth_cuts()


class _Scenes:
    """The two scenes of the script, built once and shared by every run (no run changes a parameter)."""

    def __init__(self, dev):
        from goi_hyperplane_amd.render import GaussianSet, TorchCamera
        self.dev = dev
        sc = make_scene(P, S=S, seed=6, log_scale_mean=-2.8)
        self.cam = TorchCamera(make_camera(W, H, yaw=0.1, pitch=0.05), dev)
        self.bg = torch.tensor([0.2, 0.3, 0.1], device=dev)
        g = torch.Generator(device=dev).manual_seed(0)
        self.ups = [torch.randn(s, device=dev, generator=g) for s in ((3, H, W), (S, H, W), (1, H, W), (1, H, W))]
        self.pc = GaussianSet.from_scene(sc, dev)
        self.frozen = GaussianSet.from_scene(sc, dev)  # the reference's semantic stage: only the features train
        for p in self.frozen.parameters():
            p.requires_grad_(False)
        self.frozen._semantics.requires_grad_(True)
        self.every_second = (torch.arange(P, device=dev) % 2 == 0).contiguous()
        _sc, self.cut_cam, self.cut_pc, self.cut_ups = depth_cut_setup(dev, P=200_000, seed=23)
        self.cut_bg = torch.zeros(3, device=dev)


def _frame(cam, pc, bg, ups, read_count=False, **kw):
    """One render + backward.  The outputs are copied AFTER the count was read (if it is): what a consumer would see."""
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.render import PipelineParams, render
    for p in pc.parameters():
        p.grad = None
    out = render(cam, pc, PipelineParams(), bg, **kw)
    n = rasterizer.last_num_rendered()
    if read_count:
        int(n)
    torch.autograd.backward((out["render"], out["semantics"], out["depth"], out["alpha"]), ups)
    grads = {k: p.grad.clone() for k, p in pc.named_parameters() if p.grad is not None}
    grads["means2D"] = out["viewspace_points"].grad.clone()
    return {"n": n, "out": {k: out[k].detach().clone() for k in OUTS}, "grads": grads}


def _count(rec):
    """What num_rendered is and says about its frame -- read once the test is done with leaving it unread."""
    from goi_hyperplane_amd import _C
    n = rec.pop("n")
    rec["count"] = {"type": type(n).__name__, "value": int(n)}
    if isinstance(n, _C.LazyCount):
        rec["count"].update(capacity=n.capacity, layout=n.layout, overflowed=n.overflowed, redone=n.redone,
                            cut_failed=n.cut_failed, uncut=n.cut_key is None, tiles=n.tiles)
    return rec


def _script(sc, binding):
    """-> {step: {"frames": [...], "stats": increase of every SPECULATION_STATS field, ...}}"""
    from goi_hyperplane_amd import _C
    _C.set_binding(binding)
    assert _C.binding() == binding
    _C.poll_counts(wait=True)
    _C._SPEC.clear()
    _C.forget_depth_cuts()
    _C.set_forward_mode(speculative=True, headroom=2.0, capacity=None, on_overflow="warn", max_ahead=64,
                        inference_speculative=False, min_history=3, depth_cut=False)
    log = {}
    try:
        _steps(sc, log)
    except Exception as ex:  # (every test of the file reads this log: say which step of which run could not be recorded)
        raise RuntimeError(f"the script failed under the {binding} binding in the step after {list(log)}: {ex!r}") from ex
    return log


def _steps(sc, log):
    from goi_hyperplane_amd import _C, rasterizer
    dev = sc.dev
    a = (sc.cam, sc.pc, sc.bg, sc.ups)

    def step(name, frames, **extra):
        log[name] = dict(frames=frames, stats={k: _C.SPECULATION_STATS[k] - before[k] for k in before}, **extra)

    # 1. default policy: three exact frames teach the capacity policy, two speculative ones follow
    before = dict(_C.SPECULATION_STATS)
    step("policy", [_count(_frame(*a)) for _ in range(5)])
    n0 = log["policy"]["frames"][-1]["count"]["value"]
    # 2. overflow, the count read before the outputs are used: redone in place
    before = dict(_C.SPECULATION_STATS)
    _C.set_forward_mode(capacity=n0 // 2)
    step("overflow_read", [_count(_frame(*a, read_count=True))])
    # 3. overflow, the count not read: zero gradients, a warning and a skipped view at a later poll
    before = dict(_C.SPECULATION_STATS)
    with warnings.catch_warnings(record=True) as seen:  # (the backward's free look may be the one that finds it)
        warnings.simplefilter("always")
        rec = _frame(*a)
        torch.cuda.synchronize(dev)
        _C.poll_counts(dev, wait=True)
    step("overflow_unread", [_count(rec)],
         warnings=len([w for w in seen if issubclass(w.category, _C.RasterOverflowWarning)]))
    _C.set_forward_mode(capacity=None)
    # 4. every second Gaussian, then the others: exact and speculative
    before = dict(_C.SPECULATION_STATS)
    frames = []
    for invert in (False, True):
        for spec in (False, True):
            _C.set_forward_mode(speculative=spec)
            frames.append(_count(_frame(*a, gaussian_mask=sc.every_second, in_place=True, mask_invert=invert)))
    step("selected", frames)
    # 5. a truncation window over a frame that fits and one that does not
    before = dict(_C.SPECULATION_STATS)
    word = lambda t: None if t is None else int(t.item())  # noqa: E731
    rasterizer.accumulate_truncation(dev)
    fits = _frame(*a)
    acc_fit = word(rasterizer.truncated_flag(accumulated=True))
    _C.set_forward_mode(capacity=n0 // 2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", _C.RasterOverflowWarning)
        short = _frame(*a)
        acc_short, last_short = word(rasterizer.truncated_flag(accumulated=True)), word(rasterizer.truncated_flag())
        rasterizer.reset_truncation()
        acc_reset = word(rasterizer.truncated_flag(accumulated=True))
        rasterizer.accumulate_truncation(None)
        _C.set_forward_mode(capacity=None)
        _C.poll_counts(dev, wait=True)
    step("window", [_count(fits), _count(short)], acc_fit=acc_fit, acc_short=acc_short, last_short=last_short,
         acc_reset=acc_reset, closed=rasterizer.truncated_flag(accumulated=True) is None)
    # 6. geometry cache, frozen geometry, the same camera twice
    before = dict(_C.SPECULATION_STATS)
    rasterizer.set_geometry_cache(1 << 30)
    c0 = rasterizer.geometry_cache_stats()
    frames = [_count(_frame(sc.cam, sc.frozen, sc.bg, sc.ups)) for _ in range(2)]
    c1 = rasterizer.geometry_cache_stats()
    rasterizer.set_geometry_cache(0)
    step("cache", frames, hits=c1["hits"] - c0["hits"], misses=c1["misses"] - c0["misses"],
         entries_left=rasterizer.geometry_cache_stats()["entries"])
    # 7. the depth cut: learnt, applied, then sabotaged with the count read
    before = dict(_C.SPECULATION_STATS)
    d0 = _C.depth_cut_stats()
    c = (sc.cut_cam, sc.cut_pc, sc.cut_bg, sc.cut_ups)
    frames = [_count(_frame(*c)) for _ in range(4)]
    _C.set_forward_mode(depth_cut=True)
    frames.append(_count(_frame(*c)))  # learns
    frames.append(_count(_frame(*c)))  # the first cut frame
    (entry,) = _C._DEPTH_CUTS["entries"].values()
    entry["z"].mul_(0.5)  # every learnt cut far in front of where the lists saturate
    frames.append(_count(_frame(*c, read_count=True)))
    d1 = _C.depth_cut_stats()
    _C.set_forward_mode(depth_cut=False)
    step("depth_cut", frames, cut=dict(cameras=d1["cameras"], cut_frames=d1["cut_frames"] - d0["cut_frames"],
                                       cut_failures=d1["cut_failures"] - d0["cut_failures"]))


def _exact(sc):
    """The same frames by the exact, synchronous forward (compiled binding)."""
    from goi_hyperplane_amd import _C
    _C.set_binding("compiled")
    _C.set_forward_mode(speculative=False, depth_cut=False)
    a = (sc.cam, sc.pc, sc.bg, sc.ups)
    return {"plain": _count(_frame(*a)),
            "selected": _count(_frame(*a, gaussian_mask=sc.every_second, in_place=True)),
            "unselected": _count(_frame(*a, gaussian_mask=sc.every_second, in_place=True, mask_invert=True)),
            "frozen": _count(_frame(sc.cam, sc.frozen, sc.bg, sc.ups)),
            "depth_cut": _count(_frame(sc.cut_cam, sc.cut_pc, sc.cut_bg, sc.cut_ups))}


@pytest.fixture(scope="module")
def runs(dev):
    sc = _Scenes(dev)
    try:
        return {"compiled": _script(sc, "compiled"), "ctypes": _script(sc, "ctypes"), "exact": _exact(sc)}
    finally:
        _restore()


def _same_out(a, b, where):
    for k in OUTS:
        assert torch.equal(a["out"][k], b["out"][k]), (where, k)


STEPS = ("policy", "overflow_read", "overflow_unread", "selected", "window", "cache", "depth_cut")


@pytest.mark.parametrize("name", STEPS)
def test_both_bindings_drive_the_step_alike(runs, name):
    a, b = runs["compiled"][name], runs["ctypes"][name]
    assert len(a["frames"]) == len(b["frames"])
    for i, (fa, fb) in enumerate(zip(a["frames"], b["frames"])):
        _same_out(fa, fb, (name, i))
        assert fa["grads"].keys() == fb["grads"].keys()
        for k in fa["grads"]:
            assert torch.equal(fa["grads"][k], fb["grads"][k]), (name, i, k)
        assert fa["count"] == fb["count"], (name, i)
    for k in a:  # the counters the step moved and whatever else it noted (waits: whether a count has arrived is timing)
        if k == "frames":
            continue
        va, vb = a[k], b[k]
        if k == "stats":
            va, vb = ({f: v for f, v in d.items() if f != "waits"} for d in (va, vb))
        assert va == vb, (name, k, va, vb)


@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
def test_the_default_policy_teaches_three_exact_frames_then_speculates(runs, binding):
    st = runs[binding]["policy"]
    assert st["stats"]["exact_frames"] == 3 and st["stats"]["speculative_frames"] == 2
    assert [f["count"]["type"] for f in st["frames"]] == ["int"] * 3 + ["LazyCount"] * 2
    for f in st["frames"]:
        assert f["count"]["value"] == runs["exact"]["plain"]["count"]["value"]
    for f in st["frames"][3:]:
        assert f["count"]["tiles"] == 80 and not f["count"]["overflowed"] and f["count"]["uncut"]


@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
def test_overflow_is_redone_when_read_and_a_skipped_view_when_not(runs, binding):
    n0 = runs["exact"]["plain"]["count"]["value"]
    st = runs[binding]["overflow_read"]
    (c,) = [f["count"] for f in st["frames"]]
    assert c["capacity"] == n0 // 2 and c["overflowed"] and c["redone"] and c["layout"] == n0 and c["value"] == n0
    assert st["stats"]["redone"] == 1 and st["stats"]["overflows"] == 1 and st["stats"]["skipped_views"] == 0
    st = runs[binding]["overflow_unread"]
    (f,) = st["frames"]
    assert f["count"]["overflowed"] and not f["count"]["redone"] and f["count"]["layout"] == n0 // 2
    assert all(float(g.abs().max()) == 0.0 for g in f["grads"].values())
    assert st["warnings"] == 1 and st["stats"]["skipped_views"] == 1 and st["stats"]["redone"] == 0


@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
def test_selected_frames_keep_their_kind_and_count(runs, binding):
    frames = runs[binding]["selected"]["frames"]
    assert [f["count"]["type"] for f in frames] == ["int", "LazyCount", "int", "LazyCount"]
    for f, ref in zip(frames, ("selected", "selected", "unselected", "unselected")):
        assert f["count"]["value"] == runs["exact"][ref]["count"]["value"]
        assert bool((f["out"]["radii"][1::2] == 0).all()) == (ref == "selected")
    assert all(f["count"]["uncut"] for f in frames if f["count"]["type"] == "LazyCount")


@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
def test_the_truncation_window_sees_the_frame_that_was_just_launched(runs, binding):
    """The frame's "truncated" word is OR-ed into the window BEHIND the kernels that write it: 0 after a frame that fits, the
    frame's own word after one that does not, 0 again after a reset, nothing once the window is closed."""
    st = runs[binding]["window"]
    assert st["acc_fit"] == 0
    assert st["acc_short"] != 0 and st["acc_short"] == st["last_short"]
    assert st["acc_reset"] == 0 and st["closed"]
    assert st["stats"]["skipped_views"] == 1  # (the overflowing frame's count was never read)


@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
def test_the_geometry_cache_misses_once_then_hits(runs, binding):
    st = runs[binding]["cache"]
    assert st["misses"] == 1 and st["hits"] == 1 and st["entries_left"] == 0 and st["stats"]["cached_frames"] == 1
    first, again = st["frames"]
    _same_out(first, again, "cache")
    assert torch.equal(first["grads"]["_semantics"], again["grads"]["_semantics"])


@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
def test_a_depth_cut_is_learnt_applied_and_repaired_when_it_fails(runs, binding):
    st = runs[binding]["depth_cut"]
    counts = [f["count"] for f in st["frames"]]
    assert [c["type"] for c in counts] == ["int"] * 3 + ["LazyCount"] * 4
    assert all(c["uncut"] for c in counts[3:5]) and not counts[5]["uncut"] and not counts[5]["cut_failed"]
    assert counts[5]["value"] < counts[4]["value"]  # (the cut frame lists fewer instances)
    assert not counts[6]["uncut"] and counts[6]["cut_failed"] and counts[6]["redone"]
    assert counts[6]["value"] == runs["exact"]["depth_cut"]["count"]["value"]
    assert st["stats"]["cut_failures"] == 1 and st["cut"]["cut_failures"] == 1 and st["cut"]["cut_frames"] == 2


def test_the_compiled_run_equals_exact_mode_frames(runs):
    """Every frame of the script that is not a truncated one shows the exact forward's picture."""
    run, exact = runs["compiled"], runs["exact"]
    for name, ref, which in (("policy", "plain", range(5)), ("overflow_read", "plain", [0]), ("window", "plain", [0]),
                             ("cache", "frozen", range(2)), ("depth_cut", "depth_cut", range(7))):
        for i in which:
            _same_out(run[name]["frames"][i], exact[ref], (name, i))
    for i, ref in enumerate(("selected", "selected", "unselected", "unselected")):
        _same_out(run["selected"]["frames"][i], exact[ref], ("selected", i))
    for name, i in (("overflow_unread", 0), ("window", 1)):  # (what an overflow is: the truncated picture differs)
        assert not torch.equal(run[name]["frames"][i]["out"]["render"], exact["plain"]["out"]["render"])
