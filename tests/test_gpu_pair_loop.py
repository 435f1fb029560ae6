"""The forward blend's pair loop (csrc/render_fwd.hip, apply()) on the cases its control flow can get wrong, at the smallest
shapes that reach them.  The loop accumulates under the pixel's own condition (EXEC) instead of by select, tests for the wave's
end only at a pair where a live pixel fails the transmittance test, and reads one staged record per slot.

ONE SCENE: a 24 x 20 image (one full tile, partial tiles, lanes and whole quadrants outside the image) with 70 Gaussians stacked
on tile (0, 0), 0.01 apart in depth, so that the tile's list takes two rounds of 64 and list position = index:
  * index 10: sharp, opacity 0.015, centred ON pixel (3, 4): alpha >= 1/255 at that pixel only (0.015 exp(-1 / 0.6) = 0.0028 at
    its neighbours) -- the contribution ellipse reaches exactly one pixel of quadrant 0;
  * index 20: sharp, centred BETWEEN four pixels of quadrant 0 with alpha = 0.97 / 255 at the nearest pixel centres: it passes the
    quadrant test (its centre lies inside) and contributes nowhere;
  * indices 36 .. 43: opacity 0.99, sigma 8 pixels, centred on quadrant 3: the pixels of that quadrant end one after the other in
    the middle of the first round (a live pixel that hits and fails T (1 - alpha) >= 1e-4), the wave leaves when the last one
    has; the other quadrants keep live and finished pixels side by side into the second round;
  * the rest: opacity 0.05, sigma 2.5 .. 4 pixels, spread over the tile.
That these things happen is asserted from the frame itself (the dumped pair bits, n_contrib), not assumed.
S in {16, 3, 17}: whole float4 rows, the register path of a ragged row, S4 = 5.

Checks:
  * DECISIONS: n_contrib, alpha, member masks, qcost and every image of the default forward (two candidates per trip) equal those
    of the one-candidate loop (fwd_variant 0) bit for bit, and so do all gradients; member masks, qcost and n_contrib agree with
    the float64 reference (blend_reference.check_masks / check_forward).
  * EXEC MASKING: the scene rendered with and without Gaussian 10 is bit-equal in every output channel at every pixel but (3, 4);
    with 3e38 in one of its features the same holds and everything is finite; with +inf in one semantic channel every other pixel
    stays finite (the reference `continue`s past a pixel a Gaussian does not reach).
  * AGAINST FLOAT64: pair evaluation, images and every element of every backward row within the per-element tolerances of
    tests/test_gpu_blend_rows.py, through the default (split-f16) flush and the exact-fp32 one (bwd_variant 2 = mode 1 of the
    debug hook).  The pooled gate of that file (4 x median, 99th percentile, 16 x maximum of the yardstick over ALL its cases) is
    a statement about that population and is not applied to one 70-Gaussian scene.
  * OTHER INSTANTIATIONS: a depth-cut frame (LEARN) equals the uncut frame bit for bit -- on the scene as it is (nothing to cut:
    the lists end inside the margin) and with the opaque block moved to indices 2 .. 9 and spread over the image, where tile 0
    learns a finite cut and the next frame lists fewer instances; trace() agrees with the oracle as tests/test_gpu_parity.py
    requires.

Nothing here is built to make a kernel fault: every frame is a valid forward of the product.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from goi_hyperplane_amd.scene import GaussianScene, make_camera
from tests import blend_cases as BC
from tests import blend_reference as BR

pytestmark = pytest.mark.gpu
W, H, K = 24, 20, 70
ONE_PIXEL, SUB_THRESHOLD, WALL = 10, 20, tuple(range(36, 44))
PIXEL = (3, 4)       # the pixel Gaussian ONE_PIXEL reaches
SHARP_SIGMA = 0.05   # pixels; the rasterizer's low-pass filter adds 0.3 to the 2-D variance
COV_SHARP = SHARP_SIGMA ** 2 + 0.3
BG = np.array([0.3, 0.7, 0.1], np.float32)


def pair_loop_scene(S: int, *, wall=WALL, wall_sigma=8.0, wall_centre=(11.5, 11.5)):
    cam = make_camera(W, H)
    rng = np.random.default_rng(BC.seed_of(f"pair-loop/{S}"))
    zc = 5.0 + 0.01 * np.arange(K)
    cx, cy = rng.uniform(1.0, 15.0, K), rng.uniform(1.0, 15.0, K)
    sigma = rng.uniform(2.5, 4.0, K)
    opacity = np.full(K, 0.05)
    cx[ONE_PIXEL], cy[ONE_PIXEL], sigma[ONE_PIXEL], opacity[ONE_PIXEL] = PIXEL[0], PIXEL[1], SHARP_SIGMA, 0.015
    cx[SUB_THRESHOLD], cy[SUB_THRESHOLD], sigma[SUB_THRESHOLD] = 5.5, 2.5, SHARP_SIGMA
    opacity[SUB_THRESHOLD] = 0.97 / 255.0 / np.exp(-0.5 * 0.5 / COV_SHARP)  # the nearest pixel centres are (0.5, 0.5) away
    for k in wall:
        cx[k], cy[k], sigma[k], opacity[k] = wall_centre[0], wall_centre[1], wall_sigma, 0.99
    ndc_x, ndc_y = (2 * cx + 1) / W - 1, (2 * cy + 1) / H - 1
    xyz = np.stack([ndc_x * zc * cam.tanfovx, ndc_y * zc * cam.tanfovy, zc - 5.0], 1).astype(np.float32)
    focal = W / (2 * cam.tanfovx)
    scales = np.repeat((sigma * zc / focal)[:, None], 3, 1).astype(np.float32)
    rot = np.zeros((K, 4), np.float32)
    rot[:, 0] = 1
    sc = GaussianScene(xyz, scales, rot, opacity[:, None].astype(np.float32), rng.normal(0, 0.5, (K, 1, 3)).astype(np.float32),
                       rng.normal(0, 1, (K, S)).astype(np.float32), 0)
    return sc, cam


def without(sc: GaussianScene, k: int) -> GaussianScene:
    keep = np.arange(sc.P) != k
    return GaussianScene(sc.means3D[keep], sc.scales[keep], sc.rotations[keep], sc.opacities[keep], sc.shs[keep], sc.semantics[keep],
                         sc.sh_degree)


def _frame(sc, cam):
    from tests.test_gpu_blend_rows import DeviceFrame
    return DeviceFrame(sc, cam, BG)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _lane(px, py):
    return (py & 7) * 8 + (px & 7)


_SHARED = {}


def _default_frame(S):
    """The scene's frame through the default forward, rendered once per S and left unchanged."""
    if S not in _SHARED:
        sc, cam = pair_loop_scene(S)
        _SHARED[S] = (sc, cam, _frame(sc, cam))
    return _SHARED[S]


def _pairs_of(df, k, quad):
    qd = df.quads
    sel = np.flatnonzero((qd.pair_id == k) & (qd.pair_quad == quad))
    assert len(sel) == 1, (k, quad, len(sel))
    return int(sel[0])


@pytest.mark.parametrize("S", [16, 3, 17])
def test_the_scene_reaches_the_paths_it_is_built_for(S):
    sc, cam, df = _default_frame(S)
    qd, hit = df.quads, df.hit
    assert qd.length[0] == K and np.array_equal(qd.pair_id[qd.off[0]:qd.off[1]], np.arange(K)), "tile 0 lists all 70, in depth order"
    assert (~qd.inside).all(axis=1).any() and ((~qd.inside).any(axis=1) & qd.inside.any(axis=1)).any(), "quadrants outside / partly outside"
    # the one-pixel Gaussian: one lane of quadrant 0, no lane of any other quadrant
    one = hit[_pairs_of(df, ONE_PIXEL, 0)]
    assert one.sum() == 1 and one[_lane(*PIXEL)], np.flatnonzero(one)
    others = np.flatnonzero((qd.pair_id == ONE_PIXEL) & (qd.pair_quad != 0))
    assert not hit[others].any()
    assert qd.nc[0, _lane(*PIXEL)] > ONE_PIXEL, "the pixel is live when its Gaussian comes"
    # the sub-threshold Gaussian: listed, its centre inside quadrant 0, both guards' `below` passed, `seen` nowhere
    sub = _pairs_of(df, SUB_THRESHOLD, 0)
    assert not hit[np.flatnonzero(qd.pair_id == SUB_THRESHOLD)].any()
    assert df.al[sub].max() > 0.9 / 255.0 and df.al[sub].max() < 1.0 / 255.0
    # the opaque block ends quadrant 3 in the middle of the first round, its pixels at different pairs; the wave leaves there
    nc3 = qd.nc[3]
    assert WALL[0] < nc3.min() and nc3.max() <= WALL[-1] + 1 < 64 and len(np.unique(nc3)) > 1, np.unique(nc3)
    a3 = df.alpha.cpu().numpy()[8:16, 8:16]
    assert (1.0 - a3 < 1.0e-2).all(), "quadrant 3 saturates"
    # the other quadrants of tile 0 hold finished and live pixels side by side and walk into the second round
    mixed = [q for q in (0, 1, 2) if (qd.nc[q] <= WALL[-1] + 1).any() and (qd.nc[q] > 64).any()]
    assert mixed, [np.unique(qd.nc[q]) for q in (0, 1, 2)]


@pytest.mark.parametrize("S", [16, 3, 17])
def test_decisions_and_images_equal_the_one_candidate_loop_bit_for_bit(S):
    from goi_hyperplane_amd import _lib
    from tests.test_gpu_parity import run_hip
    from tests.golden.make_golden import upstream_grads
    sc, cam, df = _default_frame(S)
    up, _ = BC.upstream("random", S, H, W, "pair-loop")
    grads = upstream_grads(S, H, W, seed=6)
    out1 = df.blend(0, up)
    res1 = run_hip(sc, cam, BG, torch.device("cuda:0"), grads=grads)
    try:
        _lib.set_option("fwd_variant", 0)
        df0 = _frame(sc, cam)
        out0 = df0.blend(0, up)
        res0 = run_hip(sc, cam, BG, torch.device("cuda:0"), grads=grads)
    finally:
        _lib.set_option("fwd_variant", 1)
    assert np.array_equal(df.frame.n_contrib, df0.frame.n_contrib)
    assert np.array_equal(out1["qcost"], out0["qcost"])
    # (member words are specified up to the quadrant's qcost: a wave that never starts a round writes none)
    look = df.quads.pair_pos < df.quads.qmax[df.quads.pair_quad]
    assert np.array_equal(BR.decode_masks(df.quads, out1["qmask0"], out1["qmask"])[look],
                          BR.decode_masks(df0.quads, out0["qmask0"], out0["qmask"])[look])
    m1, m0 = df.maps(), df0.maps()
    for k in m1:
        assert np.array_equal(_bits(m1[k]), _bits(m0[k])), k
    for k in ("radii", "alpha", "render", "semantics", "depth"):
        assert np.array_equal(res0[k], res1[k]), k
    for k, g in res0["grads"].items():
        if g is not None:
            assert np.array_equal(g, res1["grads"][k]), k
    # ... and the decisions are the float64 reference's
    BR.check_masks(df.quads, df.hit, out1["qmask0"], out1["qmask"], out1["qcost"])


def _maps_of(sc, cam):
    m = _frame(sc, cam).maps()
    return np.concatenate([m["color"], m["sem"], m["depth"][None], m["alpha"][None]], 0)  # [3 + S + 2, H, W]


@pytest.mark.parametrize("S", [16, 3, 17])
def test_a_pixel_the_gaussian_does_not_reach_is_untouched(S):
    sc, cam, df = _default_frame(S)
    m = df.maps()
    full = np.concatenate([m["color"], m["sem"], m["depth"][None], m["alpha"][None]], 0)
    assert full.shape[0] == S + 5  # (21 channels at S = 16)
    away = np.ones((H, W), bool)
    away[PIXEL[1], PIXEL[0]] = False
    bare = _maps_of(without(sc, ONE_PIXEL), cam)
    assert np.array_equal(_bits(full)[:, away], _bits(bare)[:, away])
    assert (full[:, ~away] != bare[:, ~away]).any(), "the Gaussian does contribute to its pixel"
    # a feature of 3e38: 0.015 T x 3e38 is finite; every other pixel as before, bit for bit
    big = pair_loop_scene(S)[0]
    big.semantics[ONE_PIXEL, S // 2] = 3e38
    mb = _maps_of(big, cam)
    assert np.isfinite(mb).all()
    assert np.array_equal(_bits(mb)[:, away], _bits(bare)[:, away])
    # +inf in one semantic channel: only the pixel it reaches may see it
    inf = pair_loop_scene(S)[0]
    inf.semantics[ONE_PIXEL, S - 1] = np.inf
    mi = _maps_of(inf, cam)
    assert np.isfinite(mi[:, away]).all()
    assert np.array_equal(_bits(mi)[:, away], _bits(bare)[:, away])


@pytest.mark.parametrize("S", [16, 3, 17])
def test_images_and_backward_rows_against_float64(S):
    sc, cam, df = _default_frame(S)
    fr, qd = df.frame, df.quads
    up, _ = BC.upstream("random", S, H, W, "pair-loop")
    st = BR.check_pairs(fr, qd, df.E, df.al, df.guards)
    print("pair evaluation", st)
    fw = BR.check_forward(fr, qd, BR.forward_reference(fr, qd, df.al, df.hit), df.maps(), BR.GATE)
    print("forward", fw)
    ref = BR.backward_rows(fr, qd, up, df.E, df.al, df.hit)
    ncol = BR.nsem_of(S) + 10
    for mode, what in ((0, "default flush"), (1, "exact-fp32 flush (bwd_variant 2)")):
        out = df.blend(mode, up)
        if mode == 0:
            BR.check_masks(qd, df.hit, out["qmask0"], out["qmask"], out["qcost"])
        slots = BR.slots_reference(fr, qd, out["aux"])
        BR.check_flags(slots, ref.member, out["flags"], df.N)
        got = np.zeros((qd.npairs, ncol), np.float32)
        got[ref.member] = np.asarray(out["rows"])[slots[ref.member]][:, :ncol]
        err = BR.check_rows(S, qd, ref, got, BR.GATE, f"pair-loop S={S}/{what}", split=mode == 0)
        print(what, {c: [x / BR.U for x in v[:3]] for c, v in BR.class_stats(S, err).items()})


def _step(cam, pc, ups):
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.render import PipelineParams, render
    for p in pc.parameters():
        p.grad = None
    out = render(cam, pc, PipelineParams(), torch.tensor(BG, device=cam.camera_center.device))
    n = rasterizer.last_num_rendered()
    torch.autograd.backward((out["render"], out["semantics"], out["depth"], out["alpha"]), ups)
    grads = [p.grad.clone() for p in pc.parameters()] + [out["viewspace_points"].grad.clone()]
    return out, n, grads


@pytest.mark.parametrize("early_wall", [False, True])
def test_depth_cut_frames_equal_uncut_frames(early_wall):
    """The LEARN instantiation (stop positions, the flag of a cut that is too tight).  early_wall: the opaque block at indices
    2 .. 9, sigma 100 pixels -- every pixel of the image ends inside it, tile 0 stops at a position s <= 10 and learns the depth of
    entry s + s / 8 + 32 < 70: the next frame of the camera lists less and is the same frame."""
    from goi_hyperplane_amd import _C, rasterizer
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from tests.test_gpu_depth_cut import _same_gradients
    dev = torch.device("cuda:0")
    S = 16
    sc, cam_np = pair_loop_scene(S, wall=tuple(range(2, 10)), wall_sigma=100.0) if early_wall else pair_loop_scene(S)
    cam, pc = TorchCamera(cam_np, dev), GaussianSet.from_scene(sc, dev)
    gen = torch.Generator(device=dev).manual_seed(9)
    ups = [torch.randn(shape, device=dev, generator=gen) / (W * H) for shape in ((3, H, W), (S, H, W), (1, H, W), (1, H, W))]
    _C._SPEC.clear()
    _C.forget_depth_cuts()
    rasterizer.set_forward_mode(speculative=True, depth_cut=False)
    try:
        for _ in range(4):
            ref_out, ref_n, ref_g = _step(cam, pc, ups)
        n_uncut = int(ref_n)
        rasterizer.set_forward_mode(depth_cut=True)
        _step(cam, pc, ups)                 # learns
        out1, n1, g1 = _step(cam, pc, ups)  # applies what the frame before learnt, checks it, learns again
        out2, n2, g2 = _step(cam, pc, ups)
        torch.cuda.synchronize()
        (entry,) = _C._DEPTH_CUTS["entries"].values()
        z = entry["z"].cpu().numpy()
        print("uncut", n_uncut, "cut", int(n1), int(n2), "learnt z", z)
        for out, g in ((out1, g1), (out2, g2)):
            for k in ("render", "semantics", "depth", "alpha", "radii"):
                assert torch.equal(out[k], ref_out[k]), k
            _same_gradients(g, ref_g)
        assert not n1.cut_failed and not n2.cut_failed
        if early_wall:
            assert np.isfinite(z[0]) and 5.0 < z[0] < 5.0 + 0.01 * K, z
            assert int(n1) < n_uncut and int(n2) < n_uncut, (int(n1), int(n2), n_uncut)
        else:
            assert np.isinf(z).all(), z  # (no tile of this scene stops more than 32 positions before the end of its list)
            assert int(n1) == n_uncut and int(n2) == n_uncut
    finally:
        rasterizer.set_forward_mode(depth_cut=False)
        _C.forget_depth_cuts()


def test_trace_on_the_scene_matches_the_oracle(oracle_mod):
    from goi_hyperplane_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from goi_hyperplane_amd.render import TorchCamera
    dev = torch.device("cuda:0")
    S = 16
    sc, cam = pair_loop_scene(S)
    tc = TorchCamera(cam, dev)
    img = np.random.default_rng(1).normal(size=(S, H, W)).astype(np.float32)
    o = oracle_mod.from_scene(sc, cam)
    ok = o.forward().fragile == 0
    n, color, gau_sem, num = o.trace(img)
    rs = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, torch.zeros(3, device=dev), 1.0, tc.world_view_transform,
                                       tc.full_proj_transform, sc.sh_degree, tc.camera_center, False, False)
    t = lambda a: torch.tensor(a, device=dev)  # noqa: E731
    c2, g2, n2 = GaussianRasterizer(rs).trace(t(sc.means3D), None, t(sc.opacities), shs=t(sc.shs), img_sem=t(img), scales=t(sc.scales),
                                              rotations=t(sc.rotations))
    assert ok.mean() > 0.98
    assert np.abs(c2.cpu().numpy() - color)[:, ok].max() < 1e-4
    dn = np.abs(n2.cpu().numpy() - num)
    assert num[ONE_PIXEL] == S and n2.cpu().numpy()[ONE_PIXEL] == S, "the one-pixel Gaussian (alpha 0.015 > 0.005) is traced at one pixel"
    assert (dn > 0).mean() < 0.02
    same = dn == 0
    assert np.abs(g2.cpu().numpy() - gau_sem)[same].max() < 1e-3 * max(1.0, np.abs(gau_sem).max())
