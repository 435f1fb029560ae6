"""goi_raster_contrib_frame (csrc/contrib.hip) and goi_hyperplane_amd.contrib on the GPU.

REPLAY, bit for bit: an exact forward of every case; alpha and the guard bits of EVERY candidate pair dumped with
goi_raster_debug_pair_eval, the lists with debug_views; peak (as uint32), top_id and top_w (as uint32) equal to the fp32 numpy
replay of tests/contrib_reference.py.  No pixel and no Gaussian is excluded.  Then: the empty frame, a truncated frame, the
merge over cameras in either order, a selection, free pruning (all four maps of all cameras bit-identical after
prune_unseen(min_weight=0), Adam moments of the kept rows unchanged) and pixel picking.
"""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from tests import blend_cases as BC
from tests import blend_reference as BR
from tests import contrib_reference as CR
from tests import densify_reference as DR

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAPS = ("render", "semantics", "depth", "alpha")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _u32(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _forward(cam, pc, bg, mask=None):
    """One exact forward as contrib.frame drives it -> (P, W, H, n, geom, binning, img)"""
    from goi_hyperplane_amd import _C
    import math
    P, H, W = int(pc.get_xyz.shape[0]), int(cam.image_height), int(cam.image_width)
    d = lambda t: t.detach()  # noqa: E731
    args = (bg, d(pc.get_xyz), torch.Tensor([]), d(pc.get_semantics), d(pc.get_opacity), d(pc.get_scaling), d(pc.get_rotation), 1.0,
            torch.Tensor([]), cam.world_view_transform, cam.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
            H, W, d(pc.get_features), int(pc.active_sh_degree), cam.camera_center, False, False)
    if mask is None:
        n, *_m, geom, binning, img = _C.rasterize_gaussians(*args)
    else:
        n, *_m, geom, binning, img = _C.rasterize_gaussians_selected(*args, mask, False)
    return P, W, H, int(n), geom, binning, img


def _replay_of(cam, pc, bg):
    """(device ContribFrame, numpy replay (peak, top_id, top_w), frame facts) of one view"""
    from goi_hyperplane_amd import _C, _lib, contrib
    lib = _lib.load()
    P, W, H, n, geom, binning, img = _forward(cam, pc, bg)
    got = contrib.frame_buffers(P, W, H, n, geom, binning, img)
    if n == 0:
        return got, (np.zeros(P, np.float32), np.full(W * H, -1, np.int32), np.zeros(W * H, np.float32)), dict(n=0)
    v = {k: x.cpu().numpy() for k, x in _C.debug_views(P, W, H, n, geom, binning, img).items()}
    S = int(pc.get_semantics.shape[1])
    fr = BR.Frame(W, H, S, v["means2D"], v["conic_opacity"], v["rgb"], v["depths"], np.zeros((P, S), np.float32),
                  v["point_list"].astype(np.uint32), v["ranges"].astype(np.uint32), v["n_contrib"].astype(np.uint32),
                  np.zeros(W * H, np.float32), np.zeros(3, np.float32))
    qd = BR.candidates(fr)
    req = BR.requests(qd)
    npairs = len(req)
    rq = torch.from_numpy(req.astype(np.uint32).view(np.int32)).to(DEV)
    E, al = torch.full((npairs, 64), -1.0, device=DEV), torch.full((npairs, 64), -1.0, device=DEV)
    gd = torch.full((npairs, 64), 0x40, dtype=torch.uint8, device=DEV)
    assert lib.goi_raster_debug_pair_eval(P, W, H, _ptr(geom), _ptr(rq), npairs, _ptr(E), _ptr(al), _ptr(gd), None) >= 0, _lib.last_error()
    torch.cuda.synchronize()
    gd = gd.cpu().numpy()
    assert not (gd & 0xC0).any()
    al = al.cpu().numpy()
    hit = (gd & 3) == 3
    want = CR.replay(fr, qd, al, hit)
    nc = v["n_contrib"].astype(np.int64)
    facts = dict(n=n, longest=int(qd.length.max()), stopped=bool((qd.nc.max(axis=1) < qd.length).any()), clamp=bool((al[hit] == np.float32(0.99)).any()),
                 n_contrib=nc)
    return got, want, facts


def _assert_equal(got, want, what):
    peak, tid, tw = want
    assert np.array_equal(_u32(got.peak), peak.view(np.uint32)), f"{what}: peak differs in {int((_u32(got.peak) != peak.view(np.uint32)).sum())} Gaussians"
    assert np.array_equal(got.top_id.cpu().numpy().reshape(-1), tid), f"{what}: top_id differs"
    assert np.array_equal(_u32(got.top_w).reshape(-1), tw.view(np.uint32)), f"{what}: top_w differs"


def _set(sc):
    from goi_hyperplane_amd.render import GaussianSet
    return GaussianSet.from_scene(sc, DEV)


def _cam(cam):
    from goi_hyperplane_amd.render import TorchCamera
    return TorchCamera(cam, DEV)


CASES = {name: BC.ROW_CASES[name] for name in ("sub-tile-12x10", "8mod16-72x40", "ragged-123x77", "huge-64x48", "masks-400x300",
                                               "inside-160x120")}
CASES["stack-200-0.05"] = lambda: BC.stack_scene(200, 0.05)
CASES["stack-40-0.9"] = lambda: BC.stack_scene(40, 0.9)
CASES["stack-40-1.0"] = lambda: BC.stack_scene(40, 1.0)


@pytest.mark.parametrize("name", list(CASES))
def test_replay_bit_for_bit(name):
    sc, cam = CASES[name]()
    bg = torch.zeros(3, device=DEV)
    got, want, facts = _replay_of(_cam(cam), _set(sc), bg)
    assert facts["n"] > 0, "the case renders nothing"
    _assert_equal(got, want, name)
    assert (want[0] > 0).any() and (want[1] >= 0).any()
    # a pixel's dominant contributor is one of its contributors: top_id >= 0 exactly where the forward counted any
    assert np.array_equal(want[1] >= 0, facts["n_contrib"] > 0)
    if name == "stack-200-0.05":
        assert facts["longest"] > 64, "the lists must be longer than one round of 64"
    if name == "stack-40-0.9":
        assert facts["stopped"], "some pixel must end on a stopper"
    if name == "stack-40-1.0":
        assert facts["clamp"], "the 0.99 clamp must be reached"


def test_frame_runs_the_same_forward():
    """contrib.frame (its own forward) == the entry on a frame forwarded here; want_ids=False returns no maps"""
    from goi_hyperplane_amd import contrib
    sc, cam = CASES["ragged-123x77"]()
    pc, tcam, bg = _set(sc), _cam(cam), torch.zeros(3, device=DEV)
    got, want, _ = _replay_of(tcam, pc, bg)
    f = contrib.frame(tcam, pc, bg)
    _assert_equal(f, want, "contrib.frame")
    g = contrib.frame(tcam, pc, bg, want_ids=False)
    assert g.top_id is None and g.top_w is None and torch.equal(g.peak, f.peak)


def test_empty_and_truncated_frames_merge_nothing():
    from goi_hyperplane_amd import _C, contrib
    from goi_hyperplane_amd.scene import make_camera
    sc, cam = CASES["8mod16-72x40"]()
    pc, bg = _set(sc), torch.zeros(3, device=DEV)
    P = sc.P
    before = torch.rand(P, device=DEV)
    # a camera looking away: R == 0, no launch
    away = _cam(make_camera(72, 40, target=(100.0, 0.0, 0.0)))
    peak = before.clone()
    f = contrib.frame(away, pc, bg, peak=peak)
    assert f.peak is peak and torch.equal(peak, before)
    assert bool((f.top_id == -1).all()) and not bool(f.top_w.any()) and tuple(f.top_id.shape) == (40, 72)
    # a frame whose overflow word is set: the kernel merges nothing and writes -1 / 0
    Pn, W, H, n, geom, binning, img = _forward(_cam(cam), pc, bg)
    assert n > 0
    flag = _C._flag_view(geom, Pn)
    assert int(flag.item()) == 0
    flag.fill_(1)
    try:
        f = contrib.frame_buffers(Pn, W, H, n, geom, binning, img, peak=peak)
        assert torch.equal(peak, before) and bool((f.top_id == -1).all()) and not bool(f.top_w.any())
    finally:
        flag.zero_()
    f = contrib.frame_buffers(Pn, W, H, n, geom, binning, img)
    assert bool(f.peak.any()) and bool((f.top_id >= 0).any())


def test_merge_over_cameras_is_the_bitwise_maximum_in_any_order():
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.scene import make_camera, make_scene
    sc = make_scene(3000, S=16, sh_degree=1, seed=7, log_scale_mean=-2.8)
    pc, bg = _set(sc), torch.zeros(3, device=DEV)
    cams = [_cam(make_camera(123, 77, yaw=0.2, pitch=-0.1)), _cam(make_camera(96, 80, yaw=-0.4)), _cam(make_camera(64, 48, yaw=1.1, pitch=0.2))]
    singles = [contrib.frame(c, pc, bg, want_ids=False).peak for c in cams]
    want = torch.stack([s.view(torch.int32) for s in singles]).max(dim=0).values  # (non-negative floats order like their bits)
    assert bool((want >= 0).all())
    a = contrib.peak_weights(cams, pc, bg)
    b = contrib.peak_weights(cams[::-1], pc, bg)
    c = contrib.peak_weights(cams, pc, bg)
    for got in (a, b, c):
        assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want)
    assert any(not torch.equal(s, a) for s in singles), "every camera sees the same: the merge is not exercised"


def test_selection_leaves_the_unselected_untouched():
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.render import GaussianSet
    sc, cam = CASES["ragged-123x77"]()
    pc, tcam, bg = _set(sc), _cam(cam), torch.zeros(3, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    m = torch.rand(sc.P, device=DEV, generator=g) < 0.5
    sub = GaussianSet(pc._xyz[m].detach(), pc._scaling[m].detach(), pc._rotation[m].detach(), pc._opacity[m].detach(),
                      pc._features[m].detach(), pc._semantics[m].detach(), pc.active_sh_degree)
    ps = contrib.frame(tcam, sub, bg).peak
    assert bool(ps.any())
    got = contrib.frame(tcam, pc, bg, gaussian_mask=m).peak
    want = torch.zeros(sc.P, device=DEV)
    want[m] = ps
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not bool(got[~m].any())
    # merged into an array that is not zero: the unselected rows keep what was there, the selected ones take the maximum
    start = torch.full((sc.P,), 0.25, device=DEV)
    got = contrib.frame(tcam, pc, bg, gaussian_mask=m, peak=start.clone()).peak
    assert torch.equal(got, torch.maximum(start, want))


def _model(sc, seed):
    """A reference-style model (raw parameters, SH degree 1) of a scene, with a 7-group Adam whose moments are set"""
    P = sc.P
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)  # noqa: E731
    op = np.clip(sc.opacities, 1e-4, 1 - 1e-4).astype(np.float64)
    shs = np.zeros((P, 4, 3), np.float32)
    k = min(4, sc.shs.shape[1])
    shs[:, :k] = sc.shs[:, :k]
    m = DR.Model()
    m.active_sh_degree = m.max_sh_degree = 1
    raw = {"_xyz": t(sc.means3D), "_scaling": torch.log(t(sc.scales)), "_rotation": t(sc.rotations), "_opacity": t(np.log(op / (1 - op))),
           "_features_dc": t(shs[:, :1]), "_features_rest": t(shs[:, 1:]), "_semantics": t(sc.semantics)}
    for attr, v in raw.items():
        setattr(m, attr, nn.Parameter(v.contiguous()))
    m.xyz_gradient_accum = torch.zeros(P, 1, device=DEV)
    m.denom = torch.zeros(P, 1, device=DEV)
    m.max_radii2D = torch.zeros(P, device=DEV)
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, attr)], "lr": 0.0, "name": name} for name, attr in DR.PARAMS], lr=0.0, eps=1e-15)
    g = torch.Generator(device=DEV).manual_seed(seed)
    for _ in range(2):  # (lr = 0: the parameters stay, the moments fill)
        for _, attr in DR.PARAMS:
            p = getattr(m, attr)
            p.grad = torch.randn(p.shape, device=DEV, generator=g)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    return m


def _scenes_for_pruning():
    from goi_hyperplane_amd.scene import make_camera, make_scene
    # The stack's 40 Gaussians share one footprint: in a view that shows its rim, every one of them reaches some rim pixel with
    # a small alpha and nothing is unseen.  The three cameras are therefore close-ups of its core (field of view 0.05 rad: the
    # image lies within half a sigma of the centres, alpha >= 0.7 everywhere): every pixel saturates after a few Gaussians and
    # the ones behind never meet a live pixel.
    sc, cam = BC.stack_scene(40, 0.9)
    first = tuple(float(x) for x in sc.means3D[0])
    yield "stack-40-0.9", sc, [make_camera(16, 16, fovx=0.05, target=first), make_camera(24, 16, fovx=0.05, yaw=0.01, target=first),
                               make_camera(20, 12, fovx=0.04, pitch=-0.01, target=first)], True
    sc = make_scene(3000, S=16, sh_degree=1, seed=7, log_scale_mean=-2.8)
    yield "random-3000", sc, [make_camera(123, 77, yaw=0.2, pitch=-0.1), make_camera(96, 80, yaw=-0.4), make_camera(64, 48, yaw=1.1, pitch=0.2)], False


@pytest.mark.parametrize("which", [0, 1])
def test_pruning_the_unseen_is_free(which):
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.render import PipelineParams, render
    name, sc, cams, must_prune = list(_scenes_for_pruning())[which]
    cams = [_cam(c) for c in cams]
    bg = torch.tensor([0.1, 0.3, 0.2], device=DEV)
    m = _model(sc, 5)
    P = sc.P

    def frames():
        with torch.no_grad():
            outs = [render(c, m, PipelineParams(), bg) for c in cams]
        return [{k: o[k].clone() for k in MAPS} for o in outs]

    def moments():
        return {n: tuple(m.optimizer.state[getattr(m, a)][k].clone() for k in ("exp_avg", "exp_avg_sq")) for n, a in DR.PARAMS}

    # the replay's peak over the three cameras, on the model as it is
    replay_peak = np.zeros(P, np.float32)
    for c in cams:
        got, want, _ = _replay_of(c, m, bg)
        _assert_equal(got, want, name)
        replay_peak = np.maximum(replay_peak, want[0])
    before, mom = frames(), moments()
    params = {a: getattr(m, a).detach().clone() for _, a in DR.PARAMS}
    mask = contrib.prune_unseen(m, cams, bg, min_weight=0)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (P,)
    assert np.array_equal(mask.cpu().numpy(), replay_peak <= 0)
    pruned = int(mask.sum())
    if must_prune:
        assert pruned > 0, "nothing was pruned: the test would pass vacuously"
    assert m._xyz.shape[0] == P - pruned
    after = frames()
    for i, (a, b) in enumerate(zip(before, after)):
        for k in MAPS:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{name}: camera {i}: {k} changed after pruning unseen Gaussians"
    keep = ~mask
    for n, a in DR.PARAMS:
        assert torch.equal(getattr(m, a).detach(), params[a][keep]), a
        st = m.optimizer.state[getattr(m, a)]
        assert torch.equal(st["exp_avg"], mom[n][0][keep]) and torch.equal(st["exp_avg_sq"], mom[n][1][keep]), n
    # min_weight > 0: strictly below the threshold, from the replay of the model as it is now
    kept_peak = replay_peak[keep.cpu().numpy()]
    mask2 = contrib.prune_unseen(m, cams, bg, min_weight=0.01)
    assert np.array_equal(mask2.cpu().numpy(), kept_peak < np.float32(0.01))
    assert 0 < int(mask2.sum()) < mask2.numel() or not must_prune
    # and on the model as it was: the same threshold in one step
    fresh = _model(sc, 5)
    mask3 = contrib.prune_unseen(fresh, cams, bg, min_weight=0.01)
    assert np.array_equal(mask3.cpu().numpy(), replay_peak < np.float32(0.01))
    assert fresh._xyz.shape[0] == m._xyz.shape[0] and torch.equal(fresh._xyz.detach(), m._xyz.detach())


def test_pick_reads_top_id():
    from goi_hyperplane_amd import contrib
    sc, cam = BC.stack_scene(40, 0.05, W=45, H=29, centre=(41.0, 26.0))
    pc, tcam, bg = _set(sc), _cam(cam), torch.zeros(3, device=DEV)
    f = contrib.frame(tcam, pc, bg)
    top = f.top_id.cpu().numpy()
    inside, ragged, background = (38, 22), (42, 27), (2, 2)  # ragged: the quadrant x 40..47, y 24..31 of a 45 x 29 image
    assert top[inside[1], inside[0]] >= 0 and top[ragged[1], ragged[0]] >= 0 and top[background[1], background[0]] == -1
    got = contrib.pick(tcam, pc, bg, [inside, ragged, background])
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (3,)
    assert got.cpu().tolist() == [int(top[y, x]) for x, y in (inside, ragged, background)]
    one = contrib.pick(tcam, pc, bg, ragged)
    assert one.dim() == 0 and int(one) == int(top[ragged[1], ragged[0]])
    xy = torch.tensor([inside, background], device=DEV, dtype=torch.int32)
    assert contrib.pick(tcam, pc, bg, xy).cpu().tolist() == [int(top[inside[1], inside[0]]), -1]
