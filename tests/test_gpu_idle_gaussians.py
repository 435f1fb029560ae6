"""Visible Gaussians that reached no pixel skip the per-Gaussian backward (option bwd_skip_idle; goi_raster_backward: row_mask).

A listed Gaussian that sits behind the saturation front in every tile it touches owns slots but no valid row: its record is all +0
and every gradient preprocess_bwd_k would form from it is zero.  The record-mode row reduction publishes one CONTRIBUTION byte per
listed Gaussian ("owns at least one valid row", indexed by the Gaussian's first emit-order instance) and stores no all-zero record;
preprocess_bwd_k treats a visible Gaussian whose byte is 0, or that has no tiles, like an invisible one; the binding's buffer
pool keeps a byte per row ("the chain wrote it") instead of the frame's radii.

What must hold: with the option on and off every gradient -- viewspace_points.grad included -- compares equal under IEEE equality
(torch.equal: the chain on a zero record could write -0.0 where the zero path writes +0.0, nothing else may differ), whatever
the scene, the channel count, the forward, the pool's history or the mode of the backward; and the published bytes are exactly
"some validity byte of the Gaussian's slots is set"."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from goi_hyperplane_amd.scene import make_camera, make_clustered_scene, make_scene
from tests import raw_frame
from tests.raw_frame import ptr as _ptr

pytestmark = pytest.mark.gpu

# the dense occluding scene: every Gaussian is inside the frustum, 8 instances each, the lists hundreds deep -- the CPU oracle
# finds 82 % of the visible Gaussians without any gradient (asserted below, with the same fraction on the device bytes)
DENSE = dict(P=40_000, extent=(1.2, 0.9, 1.0), log_scale_mean=-3.2, W=320, H=240, seed=11)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    from goi_hyperplane_amd import _C, _lib, rasterizer
    yield
    _lib.set_option("bwd_skip_idle", 1)
    rasterizer.set_backward_mode(sh_factored=False)
    _C.poll_counts(wait=True)
    _C.set_forward_mode(speculative=True, headroom=2.0, capacity=None, on_overflow="warn", max_ahead=64,
                        inference_speculative=False, min_history=3)


def _ext():
    from goi_hyperplane_amd import _C
    ext = _C._ext()
    assert ext is not None, "the compiled binding is not built (the pool lives there)"
    return ext


def _skip_idle(on):
    from goi_hyperplane_amd import _lib
    _lib.set_option("bwd_skip_idle", 1 if on else 0)


def _dense_scene(S=16, sh_degree=3):
    d = DENSE
    return make_scene(d["P"], S=S, sh_degree=sh_degree, seed=d["seed"], extent=d["extent"], log_scale_mean=d["log_scale_mean"])


def _ups(dev, S, W, H, seed=2):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(shape, device=dev, generator=gen) / (W * H) for shape in ((3, H, W), (S, H, W), (1, H, W), (1, H, W))]


def _grads(cam, pc, ups, hold=None):
    """one render + backward through autograd -> clones of every leaf gradient and of viewspace_points.grad, radii"""
    from goi_hyperplane_amd.render import PipelineParams, render
    for p in pc.parameters():
        p.grad = None
    out = render(cam, pc, PipelineParams(), torch.zeros(3, device=cam.camera_center.device))
    torch.autograd.backward((out["render"], out["semantics"], out["depth"], out["alpha"]), ups)
    g = [p.grad for p in pc.parameters()] + [out["viewspace_points"].grad]
    if hold is not None:
        hold.append(g)
    return [None if t is None else t.clone() for t in g], out["radii"].clone()


def _assert_equal(got, want, what=""):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, i)
        if a is not None:
            assert torch.equal(a, b), (what, i)


class RawFrame(raw_frame.RawFrame):
    """One exact forward through the C ABI with its workspaces kept, and goi_raster_backward on a scratch of the test's own."""

    def __init__(self, sc, cam, dev):
        super().__init__(sc, cam, np.zeros(3, np.float32), dev)
        assert self.N > 0, "the scene renders nothing"
        self.M = int(np.asarray(sc.shs).shape[1])
        self.tiles_touched = self.views()["tiles_touched"].cpu().numpy()

    def blend_flags(self, ups):
        """the backward blend alone (the default kernel: split-f16 flush, member masks) -> validity bytes [4 N], aux [P, 4]"""
        lib, P, S, N = self.lib, self.P, self.S, self.N
        T4 = 4 * ((self.W + 15) // 16) * ((self.H + 15) // 16)
        rf = lib.goi_raster_debug_reduce_row_floats(1, S)
        scratch = torch.full((lib.goi_raster_backward_scratch_bytes(N, S),), 0xFF, dtype=torch.uint8, device=self.dev)
        rows = torch.zeros((4 * N, rf), device=self.dev)
        flags = torch.full((4 * N,), 7, dtype=torch.uint8, device=self.dev)
        aux = torch.zeros((P, 4), dtype=torch.int32, device=self.dev)
        qmask0 = torch.zeros(T4, dtype=torch.int64, device=self.dev)
        qmask = torch.zeros(4 * (N // 64 + 2), dtype=torch.int64, device=self.dev)
        qcost = torch.zeros(T4, dtype=torch.int32, device=self.dev)
        qorder = torch.zeros(8 * ((T4 + 7) // 8), dtype=torch.int32, device=self.dev)
        r = lib.goi_raster_debug_backward_blend(
            C.byref(self.scene), N, 0, _ptr(self.geom), _ptr(self.binning), _ptr(self.img), _ptr(self.radii), _ptr(self.alpha),
            *[_ptr(u) for u in ups], _ptr(scratch), _ptr(rows), _ptr(flags), _ptr(aux), _ptr(qmask0), _ptr(qmask), _ptr(qcost),
            _ptr(qorder), None, None, None, None, None, None, None)
        from goi_hyperplane_amd import _lib
        assert r >= 0, _lib.last_error()
        torch.cuda.synchronize()
        return flags.cpu().numpy(), aux.cpu().numpy().view(np.uint32)

    def backward(self, ups, masks=True):
        """goi_raster_backward on outputs and a scratch filled with 0xFF -> (dict of the eleven arrays, contribution bytes [N]
        as they lie in the scratch, row mask [P] or None)"""
        from goi_hyperplane_amd import _lib
        lib, P, S, N, M = self.lib, self.P, self.S, self.N, self.M
        nan = lambda *s: torch.full(s, float("nan"), device=self.dev)  # noqa: E731
        o = dict(mean2D=nan(P, 3), conic=nan(P, 4), opacity=nan(P), color=nan(P, 3), semantic=nan(P, S), depth=nan(P),
                 mean3D=nan(P, 3), cov3D=nan(P, 6), sh=nan(P, M, 3), scale=nan(P, 3), rot=nan(P, 4))
        scratch = torch.full((lib.goi_raster_backward_scratch_bytes(N, S),), 0xFF, dtype=torch.uint8, device=self.dev)
        assert scratch.data_ptr() % 256 == 0
        mask = torch.full((P,), 0xEE, dtype=torch.uint8, device=self.dev) if masks else None
        r = lib.goi_raster_backward(
            C.byref(self.scene), N, 0, 0, _ptr(self.geom), _ptr(self.binning), _ptr(self.img), _ptr(self.radii), _ptr(self.alpha),
            *[_ptr(u) for u in ups], *[_ptr(o[k]) for k in ("mean2D", "conic", "opacity", "color", "semantic", "depth", "mean3D",
                                                            "cov3D", "sh", "scale", "rot")],
            _ptr(scratch), None, None, _ptr(mask), None)
        assert r >= 0, _lib.last_error()
        torch.cuda.synchronize()
        off = lib.goi_raster_debug_backward_contrib_offset(N, S)
        assert off + N <= scratch.numel()
        return o, scratch[off:off + N].cpu().numpy(), None if mask is None else mask.cpu().numpy()


WRITTEN = ("mean2D", "opacity", "color", "semantic", "mean3D", "cov3D", "sh", "scale", "rot")  # (the record path leaves conic / depth alone)


def _check_bytes_against_flags(fr, ups):
    """-> (visible, contributors): the published bytes are "some validity byte of the Gaussian's slots is set", bytes of instances
    that are nobody's first keep the 0xFF the scratch came with, the row mask says "the chain ran", and the eleven arrays compare
    equal with the option off"""
    flags, aux = fr.blend_flags(ups)
    _skip_idle(True)
    on, contrib, mask = fr.backward(ups)
    _skip_idle(False)
    off, contrib_off, mask_off = fr.backward(ups)
    _skip_idle(True)
    tt = fr.tiles_touched.astype(np.int64)
    vis = fr.radii.cpu().numpy() > 0
    listed = vis & (tt > 0)
    first = aux[:, 0].astype(np.int64)
    assert listed.any() and (first[listed] + tt[listed] <= fr.N).all()
    # "some validity byte set" per listed Gaussian, from the blend's dumped flags: instances first .. first + tt, four bytes each
    per_inst = flags.reshape(fr.N, 4).any(axis=1).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(per_inst)])
    want = np.zeros(fr.P, bool)
    want[listed] = (csum[first[listed] + tt[listed]] - csum[first[listed]]) > 0
    got = np.zeros(fr.P, np.uint8)
    got[listed] = contrib[first[listed]]
    assert np.array_equal(got[listed], want[listed].astype(np.uint8)), "a contribution byte differs from 'some validity byte set'"
    untouched = np.ones(fr.N, bool)
    untouched[first[listed]] = False
    assert (contrib[untouched] == 0xFF).all(), "a byte that is no listed Gaussian's was written"
    assert (contrib_off == 0xFF).all(), "bwd_skip_idle 0 wrote contribution bytes"
    assert np.array_equal(mask, want.astype(np.uint8)), "row mask != the contributors"
    assert np.array_equal(mask_off, vis.astype(np.uint8)), "row mask of the old path != the visible Gaussians"
    for k in WRITTEN:
        assert not torch.isnan(on[k]).any(), k  # every row was written (the outputs came filled with NaN)
        assert torch.equal(on[k], off[k]), k
    for k in ("mean2D", "opacity", "color", "semantic"):  # the blend gradients are bit-identical (both are +0 where idle)
        assert torch.equal(on[k].view(torch.int32), off[k].view(torch.int32)), k
    idle = vis & ~want
    for k in WRITTEN:  # an idle Gaussian's rows are +0.0, bit for bit
        assert not on[k].view(torch.int32)[torch.from_numpy(idle).to(on[k].device)].any(), k
    return int(vis.sum()), int(want.sum())


def test_dense_occluding_scene_most_visible_gaussians_are_idle_and_take_the_new_path(oracle_mod, dev):
    d = DENSE
    sc, cam = _dense_scene(), make_camera(d["W"], d["H"])
    # the CPU oracle first: at least a third of the visible Gaussians have all-zero gradients
    rng = np.random.default_rng(0)
    gc, gs, gd, ga = (rng.standard_normal((c, d["H"], d["W"])).astype(np.float32) / (d["W"] * d["H"]) for c in (3, 16, 1, 1))
    o = oracle_mod.from_scene(sc, cam)
    f = o.forward()
    g = o.backward(gc, gs, gd, ga)
    vis_cpu = int((f.radii > 0).sum())
    moved = np.zeros(sc.P, bool)
    for k in ("means3D", "semantics", "opacity", "scales", "rotations", "sh", "means2D"):
        moved |= (np.asarray(g[k]).reshape(sc.P, -1) != 0).any(axis=1)
    idle_cpu = 1.0 - moved.sum() / vis_cpu
    print(f"oracle: visible {vis_cpu}, with a gradient {int(moved.sum())}, idle fraction {idle_cpu:.3f}")
    assert idle_cpu >= 1 / 3
    # the device: the same fraction on the published bytes (so the path cannot go untested), bytes == flags, gradients equal
    fr = RawFrame(sc, cam, dev)
    ups = [torch.from_numpy(x).to(dev) for x in (gc, gs, gd, ga)]
    vis, contributors = _check_bytes_against_flags(fr, ups)
    print(f"device: visible {vis}, contributors {contributors}, idle fraction {1 - contributors / vis:.3f}")
    assert vis == vis_cpu
    assert 1.0 - contributors / vis >= 1 / 3
    # and through autograd and the pool
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    pc, tcam = GaussianSet.from_scene(sc, dev), TorchCamera(cam, dev)
    _skip_idle(False)
    want, _ = _grads(tcam, pc, ups)
    _skip_idle(True)
    for rep in range(3):  # (fresh buffer, then pooled ones)
        got, _ = _grads(tcam, pc, ups)
        _assert_equal(got, want, rep)


def test_clustered_scene_with_big_gaussians(dev):
    """needles and frame-filling blobs: Gaussians of more than 1024 instances go through reduce_big_k, which publishes the true byte"""
    W, H = 800, 528
    sc, cam = make_clustered_scene(100_000, S=16, seed=4), make_camera(W, H)
    fr = RawFrame(sc, cam, dev)
    print("clustered: instances", fr.N, "largest Gaussian", int(fr.tiles_touched.max()), "listed", int((fr.tiles_touched > 0).sum()))
    assert fr.tiles_touched.max() > 1024, "the scene must hold a Gaussian that takes the big path"
    vis, contributors = _check_bytes_against_flags(fr, _ups(dev, 16, W, H))
    print(f"clustered: visible {vis}, contributors {contributors}")
    assert 0 < contributors < vis
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    pc, tcam, ups = GaussianSet.from_scene(sc, dev), TorchCamera(cam, dev), _ups(dev, 16, W, H)
    _skip_idle(False)
    want, _ = _grads(tcam, pc, ups)
    _skip_idle(True)
    for rep in range(2):
        got, _ = _grads(tcam, pc, ups)
        _assert_equal(got, want, rep)


@pytest.mark.parametrize("S,sh_degree", [(10, 3), (4, 1), (24, 2)])  # 128-byte rows off the 16-channel path, 64- and 192-byte rows
def test_other_channel_counts(dev, S, sh_degree):
    d = DENSE
    sc, cam = _dense_scene(S=S, sh_degree=sh_degree), make_camera(d["W"], d["H"], yaw=0.2)
    fr = RawFrame(sc, cam, dev)
    vis, contributors = _check_bytes_against_flags(fr, _ups(dev, S, d["W"], d["H"]))
    assert 1.0 - contributors / vis >= 1 / 3


def _sequence_setup(dev, S=16):
    """a dense slab wider than the frustum: every view culls a part of it and hides most of what it sees"""
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    W, H = 320, 240
    sc = make_scene(60_000, S=S, sh_degree=3, seed=31, extent=(3.0, 2.0, 1.0), log_scale_mean=-3.1)
    pc = GaussianSet.from_scene(sc, dev)
    cams = [TorchCamera(make_camera(W, H, yaw=y, pitch=p, fovx=0.7), dev) for y, p in
            ((0.0, 0.0), (0.5, 0.1), (-0.6, -0.1), (0.05, 0.0), (2.6, 0.2), (0.0, 0.0))]  # (yaw 2.6: seen from behind)
    return pc, cams, _ups(dev, S, W, H)


def test_camera_sequence_through_the_pool_zeroes_stale_rows(dev):
    ext = _ext()
    pc, cams, ups = _sequence_setup(dev)
    ext.set_grad_pool(False)
    _skip_idle(False)
    ref = [_grads(c, pc, ups) for c in cams]
    # what the sequence must contain: contributors that become idle (visible, no gradient) and idle ones that become contributors
    moved = [(g[0] != 0).any(dim=1) for g, _ in ref]   # (dL/dmeans3D row non-zero: the Gaussian contributed)
    vis = [r > 0 for _, r in ref]
    to_idle = sum(int((moved[k] & vis[k + 1] & ~moved[k + 1]).sum()) for k in range(len(cams) - 1))
    to_work = sum(int((vis[k] & ~moved[k] & moved[k + 1]).sum()) for k in range(len(cams) - 1))
    to_culled = sum(int((moved[k] & ~vis[k + 1]).sum()) for k in range(len(cams) - 1))
    print("contributors -> idle", to_idle, "idle -> contributors", to_work, "contributors -> culled", to_culled)
    assert to_idle > 100 and to_work > 100 and to_culled > 100
    ext.set_grad_pool(True)
    try:
        for on in (True, False, True):  # (also a pool whose buffers were last written by the other path)
            _skip_idle(on)
            h0 = ext.grad_pool_stats()
            got = [_grads(c, pc, ups) for c in cams + cams]
            h1 = ext.grad_pool_stats()
            assert h1[0] - h0[0] >= len(cams), (h0, h1)  # hits: reused with rows skipped
            for k, ((g, _), (r, _)) in enumerate(zip(got, ref + ref)):
                _assert_equal(g, r, (on, k))
    finally:
        ext.set_grad_pool(True)


def test_a_held_buffer_is_never_handed_out_and_a_modified_one_is_rewritten_in_full(dev):
    ext = _ext()
    pc, cams, ups = _sequence_setup(dev)
    ext.set_grad_pool(False)
    _skip_idle(False)
    ref = [_grads(c, pc, ups)[0] for c in cams[:4]]
    _skip_idle(True)
    ext.set_grad_pool(True)
    held = []
    _grads(cams[0], pc, ups, hold=held)                   # the caller keeps the gradients of view 0 ...
    kept = [t.clone() for t in held[0]]
    g1, _ = _grads(cams[1], pc, ups)                      # ... while view 1 runs: another buffer
    _assert_equal(held[0], kept, "view 0's gradients were overwritten")
    _assert_equal(g1, ref[1], "view 1")
    held.clear()                                          # view 0's buffer is free again, untouched
    s0 = ext.grad_pool_stats()
    for p in pc.parameters():
        p.grad.add_(1.0)                                  # view 1's buffer modified in place: no row holds zeros any more
        p.grad = None
    g2, _ = _grads(cams[2], pc, ups, hold=held)           # takes one of the two free buffers and keeps it ...
    g3, _ = _grads(cams[3], pc, ups)                      # ... so this one takes the other
    s1 = ext.grad_pool_stats()
    assert s1[1] > s0[1]                                  # the modified one was counted as dirty
    _assert_equal(g2, ref[2], "view 2")
    _assert_equal(g3, ref[3], "view 3")
    _assert_equal(held[0], g2, "the held buffer of view 2 was written by view 3")


def test_accumulated_views_equal_the_serial_sum(dev):
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.dist import backward_views
    from goi_hyperplane_amd.render import PipelineParams, render
    _ext()
    pc, cams, ups4 = _sequence_setup(dev)
    cams = cams[:4]
    K, params, bg, pipe = len(cams), list(pc.parameters()), torch.zeros(3, device=dev), PipelineParams()
    ups = [tuple(u * (1.0 + 0.25 * k) for u in ups4[:2]) for k in range(K)]

    def batch():
        for p in params:
            p.grad = None
        backward_views(cams, lambda cam: render(cam, pc, pipe, bg), lambda o, k: ((o["render"], o["semantics"]), ups[k]), params,
                       streams=1, on_device=True)
        assert rasterizer.last_backward_kernel() == "full_accumulate"
        torch.cuda.synchronize()
        return [p.grad.clone() for p in params]

    _skip_idle(False)
    for p in params:
        p.grad = None
    for k in range(K):  # the serial sum: K backward calls accumulating into p.grad
        o = render(cams[k], pc, pipe, bg)
        torch.autograd.backward((o["render"], o["semantics"]), ups[k])
    serial = [p.grad.clone() for p in params]
    off = batch()
    _skip_idle(True)
    for rep in range(2):
        on = batch()
        _assert_equal(on, off, rep)  # an idle Gaussian adds nothing: the same additions in the same order
    for a, w in zip(on, serial):     # and the serial sum up to the association of the fp32 additions (tests/test_gpu_dist.py's gate)
        assert float((a - w).abs().max()) <= 4e-6 * float(w.abs().max()) + 1e-12


def test_sh_factored_mode(dev):
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    d = DENSE
    sc = _dense_scene()
    pc, ups = GaussianSet.from_scene(sc, dev), _ups(dev, 16, d["W"], d["H"])
    cams = [TorchCamera(make_camera(d["W"], d["H"], yaw=y), dev) for y in (0.0, 0.4, 0.0)]

    def run():
        out = []
        for cam in cams:
            g, _ = _grads(cam, pc, ups)
            f = rasterizer.take_sh_factor()
            assert f is not None
            out.append(g + [f["gcol"].clone()])
        return out

    rasterizer.set_backward_mode(sh_factored=True)
    _skip_idle(False)
    want = run()
    _skip_idle(True)
    got = run()
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_equal(g, w, k)
    moved = (want[0][0] != 0).any(dim=1)
    assert not got[0][-1][~moved].any(), "the colour factor of an idle Gaussian is not zero"


def test_truncated_frame_between_two_good_ones(dev):
    from goi_hyperplane_amd import _C, rasterizer
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera, render
    d = DENSE
    pc, cam = GaussianSet.from_scene(_dense_scene(), dev), TorchCamera(make_camera(d["W"], d["H"]), dev)
    ups, bg = _ups(dev, 16, d["W"], d["H"]), torch.zeros(3, device=dev)

    def step(capacity):
        _C.set_forward_mode(speculative=True, capacity=capacity)
        for p in pc.parameters():
            p.grad = None
        out = render(cam, pc, PipelineParams(), bg)
        flag = rasterizer.truncated_flag()
        torch.autograd.backward((out["render"], out["semantics"], out["depth"], out["alpha"]), ups)
        g = [p.grad.clone() for p in pc.parameters()] + [out["viewspace_points"].grad.clone()]
        torch.cuda.synchronize()
        return int(flag.item()), g

    def run():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", _C.RasterOverflowWarning)
            res = [step(1 << 22), step(5000), step(1 << 22)]  # good, TRUNCATED (never read), good again -- through the pool
            _C.poll_counts(wait=True)
        return res

    _skip_idle(False)
    want = run()
    _skip_idle(True)
    got = run()
    assert [f for f, _ in got] == [0, 1, 0] == [f for f, _ in want]
    for k, ((_, g), (_, w)) in enumerate(zip(got, want)):
        _assert_equal(g, w, k)
    assert all(float(t.abs().max()) == 0.0 for t in got[1][1]), "a truncated frame produced a non-zero gradient"
    assert any(float(t.abs().max()) > 0.0 for t in got[2][1])


@pytest.mark.parametrize("speculative", [False, True])
def test_exact_and_speculative_forward(dev, speculative):
    from goi_hyperplane_amd import _C
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    d = DENSE
    pc, ups = GaussianSet.from_scene(_dense_scene(), dev), _ups(dev, 16, d["W"], d["H"])
    cams = [TorchCamera(make_camera(d["W"], d["H"], yaw=y), dev) for y in (0.0, 0.3, -0.2, 0.0)]
    _C.set_forward_mode(speculative=speculative, capacity=None)

    def run():
        return [_grads(cam, pc, ups)[0] for cam in cams]  # (the later speculative frames are sized by the policy: capacity > count)

    _skip_idle(False)
    want = run()
    _skip_idle(True)
    got = run()
    for k, (g, w) in enumerate(zip(got, want)):
        _assert_equal(g, w, k)
