"""The trace called directly -- render_fwd_k<1, true, false, false> (csrc/render_fwd.hip) through goi_raster_trace and both
bindings -- against the exact event set of tests/trace_reference.py.

Every frame is made with _C.rasterize_gaussians_trace; goi_raster_debug_views reads records, lists, ranges and the trace's n_contrib
from the workspaces it returns, and goi_raster_debug_pair_eval evaluates every candidate pair of the frame on the trace's geometry
workspace with the function pair every blend kernel uses.  With the kernel's own alphas, guard bits and last contributors as inputs
    num_gsem == S x events                                  for EVERY Gaussian, no exclusions,
    gau_sem rows of Gaussians without events == +0,
    gau_sem == the sum, bit for bit                         for an integer-valued image (integers in [-8, 8]: every partial sum is
                                                            an integer below 2^24, exact in any order),
    |gau_sem - sum| <= gamma(n - 1) sum of magnitudes       otherwise (n events: n - 1 fp32 additions that round, in any order).
Every case also holds its pairs to blend_reference.check_pairs and its n_contrib and colour map to forward_reference /
check_forward under the committed blend_reference.GATE.  The per-case statistics go to trace_stats.json next to the other artefacts.

Nothing here is built to make a kernel fault: every frame is a valid call of the product, and the refusals are raised by the
bindings before anything is launched.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import blend_cases as BC
from tests import blend_reference as BR
from tests import preprocess_reference as PR
from tests import trace_reference as TR
from tests.test_gpu_blend_rows import DeviceFrame, _artefact_dir, _check_pairs_chunked, _dev, _ptr, pair_eval

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATS = {}
NONE = torch.Tensor([])  # the reference's marker for an absent tensor argument
REFUSAL = r"img_sem must have dimensions \(S, image_height, image_width\)"


@pytest.fixture(scope="module", autouse=True)
def _stats_file():
    t0 = time.time()
    yield
    out = _artefact_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "trace_stats.json"), "w") as fh:
        json.dump(dict(stats=STATS, module_wall_seconds=round(time.time() - t0, 1)), fh, indent=1, sort_keys=True, default=float)


@pytest.fixture(autouse=True)
def _restore():
    from goi_hyperplane_amd import _C
    _C.set_binding("compiled")  # fails loudly if lib/_goi_C.so has not been built
    yield
    _C.poll_counts(wait=True)
    _C.set_binding("compiled")


def _lib():
    from goi_hyperplane_amd import _lib
    return _lib.load()


def int_image(S, H, W, tag):
    return np.random.default_rng(BC.seed_of(f"trace/int/{tag}")).integers(-8, 9, (S, H, W)).astype(np.float32)


def scaled_image(S, H, W, tag):
    """Normal values, every channel scaled by 10^k, k = -3 .. 1."""
    rng = np.random.default_rng(BC.seed_of(f"trace/normal/{tag}"))
    return (rng.normal(size=(S, H, W)) * 10.0 ** rng.integers(-3, 2, size=(S, 1, 1))).astype(np.float32)


def cov3d_of(scales, rotations, mod=1.0):
    """[P,6] (xx, xy, xz, yy, yz, zz) of R diag(mod s)^2 R^T in float64, rounded once."""
    r, x, y, z = (np.asarray(rotations, np.float64)[:, i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    L = R * (mod * np.asarray(scales, np.float64))[:, None, :]
    Sg = L @ L.transpose(0, 2, 1)
    return np.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], -1).astype(np.float32)


class Case:
    """One scene and camera as the operator's arguments; trace() runs the product, prepare() reads the frame a run left and checks
    its pairs, n_contrib and colour; check() holds a run's gau_sem / num_gsem to the event reference."""

    def __init__(self, tag, sc, cam, bg=BC.BG0, *, colors_precomp=None, cov3D_precomp=None, scale_modifier=1.0):
        self.tag, self.sc, self.cam, self.bg = tag, sc, cam, np.asarray(bg, np.float32)
        self.P, self.W, self.H = sc.P, cam.image_width, cam.image_height
        d = lambda a: NONE if a is None else _dev(a, np.float32)  # noqa: E731
        sh = None if colors_precomp is not None else sc.shs
        geo = (None, None) if cov3D_precomp is not None else (sc.scales, sc.rotations)
        self.head = (d(self.bg), d(sc.means3D), d(colors_precomp))
        self.tail = (d(sc.opacities), d(geo[0]), d(geo[1]), float(scale_modifier), d(cov3D_precomp), d(cam.world_view_transform),
                     d(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, self.H, self.W, d(sh), sc.sh_degree, d(cam.camera_center),
                     False, False)
        self.fr = None

    def args(self, img):
        return self.head + (img if torch.is_tensor(img) else _dev(img),) + self.tail

    def trace(self, img):
        from goi_hyperplane_amd import _C
        n, color, gau, num, geom, binning, imgbuf = _C.rasterize_gaussians_trace(*self.args(img))
        torch.cuda.synchronize()
        return dict(n=int(n), color=color, gau=gau, num=num, geom=geom, binning=binning, img=imgbuf)

    def views(self, run):
        from goi_hyperplane_amd import _C
        return {k: x.cpu().numpy() for k, x in _C.debug_views(self.P, self.W, self.H, run["n"], run["geom"], run["binning"],
                                                              run["img"]).items()}

    def prepare(self, run):
        assert run["n"] > 0, f"{self.tag}: the case renders nothing"
        v = self.views(run)
        self.v = v
        # (S = 1 and a zero semantic row: a trace stages no semantics; forward_reference composites r, g, b and depth)
        self.fr = BR.Frame(self.W, self.H, 1, v["means2D"], v["conic_opacity"], v["rgb"], v["depths"], np.zeros((self.P, 1), np.float32),
                           v["point_list"].astype(np.uint32), v["ranges"].astype(np.uint32), v["n_contrib"].astype(np.uint32),
                           np.zeros(self.W * self.H, np.float32), self.bg)
        self.qd = BR.candidates(self.fr)
        E, self.al, gd = pair_eval(_lib(), self.P, self.W, self.H, run["geom"], BR.requests(self.qd))
        self.hit = (gd & 3) == 3
        self.color = run["color"].cpu().numpy()
        st = dict(N=run["n"], pairs=self.qd.npairs, pair_eval=_check_pairs_chunked(self.fr, self.qd, E, self.al, gd))
        st["forward"] = BR.check_forward(self.fr, self.qd, BR.forward_reference(self.fr, self.qd, self.al, self.hit),
                                         dict(color=self.color), BR.GATE, colour_only=True)
        STATS[self.tag] = st
        return st

    def same_frame(self, run):
        """A later run of the same scene is the same frame: same lists, same last contributors, same colour bits."""
        v = self.views(run)
        assert run["n"] == self.fr.N and np.array_equal(v["point_list"], self.v["point_list"]), f"{self.tag}: the lists changed"
        assert np.array_equal(v["n_contrib"], self.v["n_contrib"]), f"{self.tag}: n_contrib changed between two runs"
        assert np.array_equal(run["color"].cpu().numpy().view(np.uint32), self.color.view(np.uint32)), f"{self.tag}: the colour changed"

    def check(self, run, img, exact, what=""):
        S = img.shape[0]
        ref = TR.trace_reference(self.fr, self.qd, self.al, self.hit, img)
        try:
            r = TR.check_trace(ref, run["gau"].cpu().numpy(), run["num"].cpu().numpy(), S, exact)
        except AssertionError as ex:
            raise AssertionError(f"{self.tag}{what} S={S} {'integer' if exact else 'scaled'} image: {ex}") from None
        st = dict(ref.stats, S=S, exact=exact, max_ratio=r["max_ratio"])
        STATS[f"{self.tag}{what}/S{S}/{'int' if exact else 'scaled'}"] = st
        print(self.tag + what, json.dumps(st), flush=True)
        return ref

    def both_images(self, S, first=False):
        """An integer-valued and a scaled normal image on this case; the first run of a case supplies the frame."""
        refs = []
        for exact, make in ((True, int_image), (False, scaled_image)):
            img = make(S, self.H, self.W, self.tag)
            run = self.trace(img)
            if self.fr is None:
                self.prepare(run)
            else:
                self.same_frame(run)
            refs.append(self.check(run, img, exact))
        return refs


# ---- channel counts on ragged images ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(123, 77), (70, 50), (50, 37), (17, 17), (5, 3)])
def test_every_channel_count_on_ragged_images(W, H):
    sc, cam = BC._rand(600, 4, W, H, -2.5, yaw=0.2, pitch=-0.1)()
    case = Case(f"channels-{W}x{H}", sc, cam)
    for S in (1, 3, 4, 10, 16, 17, 32):
        ref = case.both_images(S)[0]
        assert ref.stats["lanes_outside"] > 0 and ref.stats["events"] > 0, ref.stats
    if (W, H) == (123, 77):
        assert ref.stats["events_at_64_or_later"] > 0 and ref.stats["low_alpha_contributors"] > 0, ref.stats


# ---- stacks: the 64-position batch and pixels that stop inside one ----------------------------------------------------------------
@pytest.mark.parametrize("opacity", [0.05, 0.9])
def test_stacks_across_the_batch_of_64(opacity):
    for K in BC.STACK_K:
        sc, cam = BC.stack_scene(K, opacity)
        case = Case(f"stack-{K}-{opacity}", sc, cam)
        st = case.both_images(4)[0].stats
        assert st["events"] > 0, st
        if opacity == 0.05 and K >= 65:  # 0.95^64 = 0.04: the centre pixels are live far beyond the first batch
            assert st["events_at_64_or_later"] > 0, st
        if opacity == 0.9 and K >= 7:    # 0.1^5 < 1e-4: the centre pixels stop at the fifth Gaussian at the latest
            assert st["hits_behind_n_contrib"] > 0, st


OPACITY_EDGES = (0.0045, float(np.float32(0.005)), float(np.nextafter(np.float32(0.005), np.float32(1))), 0.0051, 0.99, 1.0)


@pytest.mark.parametrize("opacity", OPACITY_EDGES)
def test_opacity_at_the_event_threshold(opacity):
    """A stack of 9 at one opacity.  0.0045 and fp32(0.005) = 0.00499999988... lie below the double 0.005: colour, no event at all."""
    sc, cam = BC.stack_scene(9, opacity)
    assert (sc.opacities == np.float32(opacity)).all()
    case = Case(f"edge-{opacity!r}", sc, cam, BC.BG1)
    refs = case.both_images(3)
    st = refs[0].stats
    if opacity <= float(np.float32(0.005)):
        run = case.trace(int_image(3, case.H, case.W, "edge"))
        largest = float(case.al.max())
        assert st["low_alpha_contributors"] > 0, st
        assert not run["num"].any().item() and not run["gau"].view(torch.int32).any().item(), \
            f"opacity {opacity!r}: {st['events']} events; the largest alpha the kernel evaluates is {largest!r}"
    elif opacity >= 0.0051:  # (one ulp above fp32(0.005) the kernel's own rounding of alpha decides; the reference follows it)
        assert st["events"] > 0, st


# ---- a camera inside the cloud ---------------------------------------------------------------------------------------------------
def test_camera_inside_the_cloud():
    from goi_hyperplane_amd import _C
    from goi_hyperplane_amd.scene import GaussianScene, make_camera
    inp = PR.make_inputs(3000, "inside")
    cam = make_camera(**PR.POSES["inside"])
    sc = GaussianScene(inp["means3D"], inp["scales"], inp["rotations"], inp["opacities"], inp["shs"], inp["semantics"], inp["sh_degree"])
    case = Case("inside-200x152", sc, cam, BC.BG1)
    S = 4
    img = scaled_image(S, case.H, case.W, case.tag)
    run = case.trace(img)
    case.prepare(run)
    ref = case.check(run, img, False)
    vis = _C.mark_visible(case.head[1], case.tail[5], case.tail[6]).cpu().numpy()
    listed = np.bincount(case.fr.point_list.astype(np.int64), minlength=sc.P) > 0
    pv = np.c_[sc.means3D.astype(np.float64), np.ones(sc.P)] @ cam.world_view_transform.astype(np.float64)
    clamped = vis & ((np.abs(pv[:, 0] / pv[:, 2]) > 1.3 * cam.tanfovx) | (np.abs(pv[:, 1] / pv[:, 2]) > 1.3 * cam.tanfovy))
    assert (~vis).sum() > 100 and not listed[~vis].any(), "a Gaussian behind the near plane is listed"
    assert (clamped & listed).sum() > 0 and (ref.count[clamped] > 0).any(), "no clamped Gaussian takes part"
    assert not run["gau"].cpu().numpy()[~vis].view(np.uint32).any() and not run["num"].cpu().numpy()[~vis].any()
    assert ref.stats["events"] > 0 and ref.stats["events_at_64_or_later"] > 0, ref.stats


# ---- routing: precomputed colours / covariances, scale_modifier, background, both bindings -----------------------------------------
def test_routing_of_the_optional_inputs_through_both_bindings():
    from goi_hyperplane_amd import _C
    sc, cam = BC._rand(600, 4, 70, 50, -2.5, yaw=0.2, pitch=-0.1)()
    S = 10
    col = np.random.default_rng(5).uniform(0, 1, (sc.P, 3)).astype(np.float32)
    a = Case("routing/colors+modifier", sc, cam, BC.BG1, colors_precomp=col, scale_modifier=0.7)
    b = Case("routing/cov3D", sc, cam, BC.BG1, cov3D_precomp=cov3d_of(sc.scales, sc.rotations, 0.7), scale_modifier=0.7)
    plain = Case("routing/plain", sc, cam, BC.BG1)
    runs = {}
    for name in ("compiled", "ctypes"):
        _C.set_binding(name)
        assert _C.binding() == name
        for case in (a, b, plain):
            for exact, make in ((True, int_image), (False, scaled_image)):
                img = make(S, case.H, case.W, "routing")
                run = case.trace(img)
                if case.fr is None:
                    case.prepare(run)
                else:
                    case.same_frame(run)  # (the second binding leaves the first one's frame)
                case.check(run, img, exact, "/" + name)
                runs[(case.tag, name, exact)] = run
    for case in (a, b, plain):  # integer image: no order noise, the two bindings' results are the same bits
        x, y = runs[(case.tag, "compiled", True)], runs[(case.tag, "ctypes", True)]
        assert torch.equal(x["gau"], y["gau"]) and torch.equal(x["num"], y["num"]) and torch.equal(x["color"], y["color"])
    # (the records of a Gaussian that is listed nowhere are not written: compare the listed ones)
    # precomputed colours are the records' colours as they are; the modifier shrinks the footprints; the covariance of the
    # modified scales, formed in float64, gives the records the kernel's own covariance gives within fp32 noise
    sa, sb, sp = (c.v["tiles_touched"] > 0 for c in (a, b, plain))
    seen = sa & sb & sp
    assert seen.sum() > 100 and a.fr.N < plain.fr.N
    assert np.array_equal(a.v["rgb"][sa].view(np.uint32), col[sa].view(np.uint32))
    assert not np.array_equal(b.v["rgb"][seen], a.v["rgb"][seen]) and np.array_equal(b.v["rgb"][seen], plain.v["rgb"][seen])
    assert np.array_equal(a.v["means2D"][seen], plain.v["means2D"][seen])
    assert np.allclose(a.v["conic_opacity"][seen], b.v["conic_opacity"][seen], rtol=1e-3, atol=1e-6)
    assert not np.allclose(a.v["conic_opacity"][seen], plain.v["conic_opacity"][seen], rtol=1e-3, atol=1e-6)


# ---- two images per frame ----------------------------------------------------------------------------------------------------------
def test_two_images_per_frame_exact_and_bounded():
    sc, cam = BC._rand(600, 4, 123, 77, -2.5, yaw=0.2, pitch=-0.1)()
    case = Case("two-images-123x77", sc, cam)
    S = 10
    ints = int_image(S, case.H, case.W, case.tag)
    r1, r2 = case.trace(ints), case.trace(ints)
    case.prepare(r1)
    case.same_frame(r2)
    ref = case.check(r1, ints, True)
    assert ref.stats["max_events_of_a_gaussian"] > 64 and float(ref.abs_sum.max()) < 2.0 ** 24
    assert torch.equal(r1["gau"].view(torch.int32), r2["gau"].view(torch.int32)) and torch.equal(r1["num"], r2["num"])
    img = scaled_image(S, case.H, case.W, case.tag)
    assert len(np.unique(np.round(np.log10(np.abs(img).reshape(S, -1).max(axis=1))))) >= 3, "the channels share one scale"
    r3 = case.trace(img)
    case.same_frame(r3)
    case.check(r3, img, False)


# ---- against the forward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rand-123x77", "stack-129", "opaque-65"])
def test_trace_and_forward_agree_bit_for_bit(name):
    """The trace is the forward blend without the semantic channels: same pair function, same order, same stop rule -- its n_contrib
    and its colour map equal the forward's bit for bit."""
    sc, cam = dict([("rand-123x77", BC._rand(600, 16, 123, 77, -2.5, yaw=0.2, pitch=-0.1)), ("stack-129", lambda: BC.stack_scene(129, 0.05)),
                    ("opaque-65", lambda: BC.stack_scene(65, 0.9))])[name]()
    case = Case(f"forward/{name}", sc, cam, BC.BG1)
    img = scaled_image(4, case.H, case.W, case.tag)
    run = case.trace(img)
    case.prepare(run)
    case.check(run, img, False)
    df = DeviceFrame(sc, cam, BC.BG1)
    assert df.N == run["n"] and np.array_equal(df.frame.point_list, case.fr.point_list)
    assert np.array_equal(df.frame.n_contrib, case.fr.n_contrib), "the trace's and the forward's last contributors differ"
    fwd = df.color.cpu().numpy()
    diff = fwd.view(np.uint32) != case.color.view(np.uint32)
    assert not diff.any(), (f"{int(diff.sum())} colour values differ between the trace and the forward, the largest by "
                            f"{float(np.abs(fwd - case.color).max()):.3e}")


# ---- clearing ----------------------------------------------------------------------------------------------------------------------
def test_outputs_are_cleared_by_the_library():
    """goi_raster_trace through ctypes on outputs pre-filled with 0xFF bytes (NaN / -1): the results are those of clean outputs."""
    from goi_hyperplane_amd import _C, _lib
    sc, cam = BC._rand(600, 4, 70, 50, -2.5, yaw=0.2, pitch=-0.1, distance=2.0)()  # (close: part of the cloud is out of view)
    case = Case("clearing-70x50", sc, cam, BC.BG1)
    S = 5
    ints = int_image(S, case.H, case.W, case.tag)
    clean = case.trace(ints)
    case.prepare(clean)
    ref = case.check(clean, ints, True)
    assert (ref.count == 0).sum() > 10, "no Gaussian without events: nothing would show a stale row"
    lib = _lib.load()
    P, H, W = case.P, case.H, case.W
    t = dict(bg=_dev(BC.BG1), means3D=_dev(sc.means3D), shs=_dev(sc.shs), opacity=_dev(sc.opacities), scales=_dev(sc.scales),
             rotations=_dev(sc.rotations), view=_dev(cam.world_view_transform), proj=_dev(cam.full_proj_transform),
             campos=_dev(cam.camera_center), img=_dev(ints))
    scene = _C._scene(P, S, H, W, t["bg"], t["means3D"], t["shs"], None, None, t["opacity"], t["scales"], t["rotations"], 1.0, None,
                      t["view"], t["proj"], cam.tanfovx, cam.tanfovy, sc.sh_degree, t["campos"], False, False)
    ff = lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)  # noqa: E731
    color, gau, num = ff(3 * H * W * 4), ff(P * S * 4), ff(P * 4)
    geom, imgbuf = ff(lib.goi_raster_geom_bytes(P)), ff(lib.goi_raster_image_bytes(W, H))
    radii = torch.empty((P,), dtype=torch.int32, device=DEV)
    alloc = _C._BinningAllocator(torch.device(DEV, 0))
    n = lib.goi_raster_trace(C.byref(scene), _ptr(t["img"]), _ptr(geom), _ptr(imgbuf), alloc.cb, None, _ptr(color), _ptr(gau), _ptr(num),
                             _ptr(radii), None)
    if alloc.error is not None:
        raise alloc.error
    assert n >= 0, _lib.last_error()
    torch.cuda.synchronize()
    run = dict(n=n, color=color.view(torch.float32).view(3, H, W), gau=gau.view(torch.float32).view(P, S), num=num.view(torch.int32),
               geom=geom, binning=alloc.tensor, img=imgbuf)
    case.same_frame(run)
    case.check(run, ints, True, "/prefilled")
    assert torch.equal(run["gau"].view(torch.int32), clean["gau"].view(torch.int32)) and torch.equal(run["num"], clean["num"])


# ---- degenerate frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
def test_no_gaussians_and_nothing_in_view(binding):
    from goi_hyperplane_amd import _C
    from goi_hyperplane_amd.scene import GaussianScene
    _C.set_binding(binding)
    sc, cam = BC._rand(64, 4, 50, 37, -2.5)()
    S = 3
    img = scaled_image(S, 37, 50, "degenerate")
    empty = GaussianScene(*[np.zeros((0,) + np.asarray(a).shape[1:], np.float32) for a in (sc.means3D, sc.scales, sc.rotations, sc.opacities,
                                                                                            sc.shs, sc.semantics)], sc.sh_degree)
    run = Case("degenerate/P0", empty, cam, BC.BG1).trace(img)
    assert run["n"] == 0 and tuple(run["color"].shape) == (3, 37, 50) and not run["color"].view(torch.int32).any().item()
    assert tuple(run["gau"].shape) == (0, S) and tuple(run["num"].shape) == (0,) and run["num"].dtype == torch.int32
    behind = GaussianScene(sc.means3D + np.array([0, 0, -25], np.float32), sc.scales, sc.rotations, sc.opacities, sc.shs, sc.semantics,
                           sc.sh_degree)
    run = Case("degenerate/behind", behind, cam, BC.BG1).trace(img)
    want = np.broadcast_to(BC.BG1[:, None, None], (3, 37, 50))
    assert run["n"] == 0 and np.array_equal(run["color"].cpu().numpy(), want), "nothing in view: the colour is the background"
    assert tuple(run["gau"].shape) == (64, S) and not run["gau"].view(torch.int32).any().item() and not run["num"].any().item()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["compiled", "ctypes", "extension"])
def test_a_wrong_img_sem_is_refused_before_any_launch(binding):
    """An image of fewer than S H W floats would be read out of bounds: the operator under both bindings AND the compiled
    extension called directly, as the reference calls its own (the operator's Python check never runs then), refuse it by shape
    with one message, and a float64 or host image by type / device, before anything is launched."""
    from goi_hyperplane_amd import _C
    _C.set_binding("compiled" if binding == "extension" else binding)
    sc, cam = BC._rand(64, 4, 50, 37, -2.5)()
    case = Case("refusals", sc, cam)
    if binding == "extension":
        ext = _C._ext()
        assert ext is not None

        def trace(img):
            n, color, gau, num, geom, binning, imgbuf = ext.rasterize_gaussians_trace(*case.args(img))
            torch.cuda.synchronize()
            return dict(n=int(n), gau=gau)
    else:
        trace = case.trace
    H, W, S = case.H, case.W, 3
    z = lambda *shape, **kw: torch.zeros(shape, **dict(dict(device=DEV), **kw))  # noqa: E731
    for bad in (z(S, H - 1, W), z(S, H * W), z(33, H, W), z(S, H, W + 1), z(S, W, H), z(1, S, H, W), z(H, W)):
        with pytest.raises(RuntimeError, match=REFUSAL):
            trace(bad)
    with pytest.raises(TypeError, match="img_sem"):
        trace(z(S, H, W, dtype=torch.float64))
    with pytest.raises(ValueError, match="img_sem"):
        trace(z(S, H, W, device="cpu"))
    run = trace(z(S, H, W))  # (and the right one is taken)
    assert run["n"] > 0 and not run["gau"].any().item()
