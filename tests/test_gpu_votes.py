"""goi_raster_contrib_votes (csrc/contrib.hip) and the votes layer of goi_hyperplane_amd.contrib on the GPU.

BIT FOR BIT: an exact forward of every case of test_gpu_contrib.py; alpha and the guard bits of EVERY candidate pair dumped with
goi_raster_debug_pair_eval, the lists with debug_views; the int64 votes equal to the fp32 numpy replay of tests/votes_reference.py
under four label maps, each with and without ignored values.  No pixel, Gaussian or label is excluded.  Then: consistency with
peak / top_id, the backward with a one-hot upstream (an independent device path), accumulation over calls and cameras in any
order, the empty frame, a truncated frame, a selection, frame_votes, assign / lift_mask against numpy, and lift_mask on
relevant_cameras' own masks.
"""

import numpy as np
import pytest
import torch

from tests import blend_reference as BR
from tests import test_gpu_contrib as TG
from tests import votes_reference as VR

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = TG.CASES
BWD_TOL = 1e-3  # oracle/compare.py's per-tensor gate, which the backward is held to
_DUMPS = {}


def _dump(name):
    """One exact forward of a case and everything the replay needs, made once and shared (nothing in it is changed):
    dict(frame=(P, W, H, n, geom, binning, img), fr, qd, al, hit, contribs, pc, cam, facts)"""
    if name in _DUMPS:
        return _DUMPS[name]
    from goi_hyperplane_amd import _C, _lib
    lib = _lib.load()
    sc, cam = CASES[name]()
    pc, tcam, bg = TG._set(sc), TG._cam(cam), torch.zeros(3, device=DEV)
    P, W, H, n, geom, binning, img = TG._forward(tcam, pc, bg)
    assert n > 0, "the case renders nothing"
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
    assert lib.goi_raster_debug_pair_eval(P, W, H, TG._ptr(geom), TG._ptr(rq), npairs, TG._ptr(E), TG._ptr(al), TG._ptr(gd), None) >= 0, _lib.last_error()
    torch.cuda.synchronize()
    gd = gd.cpu().numpy()
    assert not (gd & 0xC0).any()
    al = al.cpu().numpy()
    hit = (gd & 3) == 3
    facts = dict(longest=int(qd.length.max()), stopped=bool((qd.nc.max(axis=1) < qd.length).any()),
                 clamp=bool((al[hit] == np.float32(0.99)).any()))
    _DUMPS[name] = dict(frame=(P, W, H, n, geom, binning, img), fr=fr, qd=qd, al=al, hit=hit,
                        contribs=VR.contributions(fr, qd, al, hit, np.float32), pc=pc, cam=tcam, bg=bg, facts=facts)
    return _DUMPS[name]


def _labels(lab):
    return torch.from_numpy(np.ascontiguousarray(lab)).to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_votes_bit_for_bit(name):
    from goi_hyperplane_amd import contrib
    d = _dump(name)
    P, W, H = d["frame"][:3]
    facts = d["facts"]
    if name == "stack-200-0.05":
        assert facts["longest"] > 64, "the lists must be longer than one round of 64"
    if name == "stack-40-0.9":
        assert facts["stopped"], "some pixel must end on a stopper"
    if name == "stack-40-1.0":
        assert facts["clamp"], "the 0.99 clamp must be reached"
    for kind in VR.MAP_KINDS:
        for ignored in (False, True):
            lab, K = VR.label_map(kind, W, H, ignored)
            want = VR.scatter(d["contribs"], lab, K, P)
            got = contrib.votes_buffers(*d["frame"], _labels(lab).reshape(H, W), K)
            assert got.dtype == torch.int64 and tuple(got.shape) == (P, K) and got.is_cuda
            got = got.cpu().numpy()
            bad = got != want
            assert not bad.any(), (f"{name} / {kind} / ignored={ignored}: {int(bad.sum())} of {bad.size} votes differ, the largest by "
                                   f"{int(np.abs(got - want).max())} units")
            assert want.any(), f"{name} / {kind}: nothing voted"
            if kind == "half-plane" and not ignored:
                ql = VR.quad_labels(d["qd"], lab, K)
                assert (((ql == 0).any(axis=1)) & ((ql == 1).any(axis=1))).any(), "some quadrant must hold two labels"
            if ignored and W * H >= 1000:
                assert all((lab == v).any() for v in (-1, K, VR.INT_MAX, VR.INT_MIN))


@pytest.mark.parametrize("name", list(CASES))
def test_votes_agree_with_peak_and_top(name):
    from goi_hyperplane_amd import contrib
    d = _dump(name)
    P, W, H = d["frame"][:3]
    f = contrib.frame_buffers(*d["frame"])
    peak = f.peak.cpu().numpy()
    uni = contrib.votes_buffers(*d["frame"], torch.zeros(H * W, dtype=torch.int32, device=DEV), 1).cpu().numpy()
    voted = uni[:, 0] > 0
    assert (peak[voted] > 0).all(), "a Gaussian with a vote must have a peak"
    contributed = np.zeros(P, bool)
    contributed[d["contribs"][1]] = True
    assert np.array_equal(voted, contributed), "K = 1, uniform: a vote exactly where the replay has a contribution"
    # the pixel's dominant contributor has a vote for that pixel's label
    lab, K = VR.label_map("64-distinct", W, H, True)
    v = contrib.votes_buffers(*d["frame"], _labels(lab), K).cpu().numpy()
    top = f.top_id.cpu().numpy().reshape(-1)
    has = (top >= 0) & (lab >= 0) & (lab < K)
    assert has.any() and (v[top[has], lab[has]] > 0).all()
    assert np.array_equal(v.sum(1) > 0, VR.scatter(d["contribs"], lab, K, P).sum(1) > 0)


@pytest.mark.parametrize("name", ["ragged-123x77", "stack-40-0.9"])
def test_votes_against_the_backward(name):
    """dL/dsemantics[g, l] of a one-hot upstream (channel l on the pixels labelled l, zero on ignored pixels) is the sum of w
    over g's contributions to those pixels: the votes in units of 2^-24, up to the backward's own tolerance and the worst-case
    quantisation of half a unit per pixel."""
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.render import PipelineParams, render
    sc, cam = CASES[name]()
    pc, tcam, bg = TG._set(sc), TG._cam(cam), torch.zeros(3, device=DEV)
    P, H, W = sc.P, int(tcam.image_height), int(tcam.image_width)
    S = int(pc.get_semantics.shape[1])
    K = 16
    assert K <= S
    y, x = np.mgrid[0:H, 0:W]
    lab = ((x % 4) + 4 * (y % 4)).reshape(-1).astype(np.int64)
    rng = np.random.default_rng(4)
    lab = np.where(rng.random(W * H) < 0.1, rng.choice(np.array([-1, K, VR.INT_MAX, VR.INT_MIN]), W * H), lab).astype(np.int32)
    valid = (lab >= 0) & (lab < K)
    G = np.zeros((S, H * W), np.float32)
    G[lab[valid], np.flatnonzero(valid)] = 1.0
    out = render(tcam, pc, PipelineParams(), bg)
    assert tuple(out["semantics"].shape) == (S, H, W)
    out["semantics"].backward(torch.from_numpy(G.reshape(S, H, W)).to(DEV))
    grad = pc._semantics.grad.detach().cpu().numpy().astype(np.float64)
    assert not grad[:, K:].any() and grad.max() > 0
    v = contrib.frame_votes(tcam, pc, bg, _labels(lab), K).cpu().numpy()
    err = np.abs(v.astype(np.float64) * 2.0 ** -24 - grad[:, :K])
    bound = BWD_TOL * np.abs(grad).max() + W * H * 2.0 ** -25
    print(f"{name}: max |votes 2^-24 - grad| = {err.max():.3e}, bound {bound:.3e}, max |grad| = {np.abs(grad).max():.3e}")
    assert (err <= bound).all(), f"{name}: {err.max():.3e} > {bound:.3e}"
    if name == "stack-40-0.9":
        # the stopper is excluded: counting it would add its w at every stopped pixel -- far more than the bound
        d = _dump(name)
        assert d["facts"]["stopped"]
        assert np.array_equal(v, VR.scatter(d["contribs"], lab, K, P))


def test_the_call_adds():
    from goi_hyperplane_amd import contrib
    d = _dump("ragged-123x77")
    P, W, H = d["frame"][:3]
    lab, K = VR.label_map("half-plane", W, H, True)
    lab = _labels(lab)
    once = contrib.votes_buffers(*d["frame"], lab, K)
    assert bool(once.any())
    twice = contrib.votes_buffers(*d["frame"], lab, K, votes=once.clone())
    assert torch.equal(twice, 2 * once)
    g = torch.Generator(device=DEV).manual_seed(9)
    start = torch.randint(-2 ** 40, 2 ** 40, (P, K), dtype=torch.int64, device=DEV, generator=g)
    arr = start.clone()
    got = contrib.votes_buffers(*d["frame"], lab, K, votes=arr)
    assert got is arr and torch.equal(arr, start + once)
    for bad in (torch.zeros(P, K, dtype=torch.int32, device=DEV), torch.zeros(P, K + 1, dtype=torch.int64, device=DEV),
                torch.zeros(K, P, dtype=torch.int64, device=DEV).t()):
        with pytest.raises(ValueError, match="votes must be a contiguous int64 tensor"):
            contrib.votes_buffers(*d["frame"], lab, K, votes=bad)
    with pytest.raises(ValueError, match="labels must be an integer or bool tensor"):
        contrib.votes_buffers(*d["frame"], lab.float(), K)
    # bool and int64 label maps are taken as they come
    m = lab == 1
    assert torch.equal(contrib.votes_buffers(*d["frame"], m, 2), contrib.votes_buffers(*d["frame"], m.to(torch.int64).reshape(H, W), 2))


def test_sweep_over_cameras_is_identical_in_any_order():
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.scene import make_camera, make_scene
    sc = make_scene(3000, S=16, sh_degree=1, seed=7, log_scale_mean=-2.8)
    pc, bg = TG._set(sc), torch.zeros(3, device=DEV)
    cams = [TG._cam(make_camera(123, 77, yaw=0.2, pitch=-0.1)), TG._cam(make_camera(96, 80, yaw=-0.4)), TG._cam(make_camera(64, 48, yaw=1.1, pitch=0.2))]
    K = 2
    labs = [_labels(VR.label_map(kind, c.image_width, c.image_height, True)[0]).reshape(c.image_height, c.image_width)
            for kind, c in zip(("half-plane", "checkerboard", "half-plane"), cams)]
    singles = [contrib.frame_votes(c, pc, bg, l, K) for c, l in zip(cams, labs)]
    want = singles[0] + singles[1] + singles[2]
    a = contrib.votes(cams, pc, bg, labs, K)
    b = contrib.votes(cams[::-1], pc, bg, labs[::-1], K)
    c = contrib.votes(cams, pc, bg, labs, K)
    for got in (a, b, c):
        assert got.dtype == torch.int64 and tuple(got.shape) == (sc.P, K) and torch.equal(got, want)
    assert not torch.equal(singles[0], singles[1]) and bool(singles[2].any())
    assert torch.equal(contrib.votes(cams, pc, bg, labs, K, votes=a.clone()), 2 * want)  # swept twice
    # a [V,H,W] and a [V,1,H,W] tensor for cameras of one size
    same = [cams[0], TG._cam(make_camera(123, 77, yaw=-0.3))]
    stack = torch.stack([labs[0], labs[0].flip(1)])
    s = contrib.votes(same, pc, bg, stack, K)
    assert torch.equal(s, contrib.votes(same, pc, bg, stack[:, None], K)) and torch.equal(s, contrib.votes(same, pc, bg, list(stack), K))
    with pytest.raises(ValueError, match="2 label maps for 3 cameras"):
        contrib.votes(cams, pc, bg, labs[:2], K)


def test_empty_and_truncated_frames_add_nothing():
    from goi_hyperplane_amd import _C, contrib
    from goi_hyperplane_amd.scene import make_camera
    sc, cam = CASES["8mod16-72x40"]()
    pc, bg = TG._set(sc), torch.zeros(3, device=DEV)
    P, K = sc.P, 2
    g = torch.Generator(device=DEV).manual_seed(1)
    before = torch.randint(-2 ** 40, 2 ** 40, (P, K), dtype=torch.int64, device=DEV, generator=g)
    lab = _labels(VR.label_map("checkerboard", 72, 40)[0])
    away = TG._cam(make_camera(72, 40, target=(100.0, 0.0, 0.0)))  # a camera looking away: R == 0, no launch
    arr = before.clone()
    assert TG._forward(away, pc, bg)[3] == 0
    assert contrib.frame_votes(away, pc, bg, lab, K, votes=arr) is arr and torch.equal(arr, before)
    Pn, W, H, n, geom, binning, img = TG._forward(TG._cam(cam), pc, bg)
    assert n > 0
    flag = _C._flag_view(geom, Pn)
    assert int(flag.item()) == 0
    flag.fill_(1)
    try:
        contrib.votes_buffers(Pn, W, H, n, geom, binning, img, lab, K, votes=arr)
        assert torch.equal(arr, before)
    finally:
        flag.zero_()
    contrib.votes_buffers(Pn, W, H, n, geom, binning, img, lab, K, votes=arr)
    assert not torch.equal(arr, before)


def test_selection_leaves_the_unselected_untouched():
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.render import GaussianSet
    sc, cam = CASES["ragged-123x77"]()
    pc, tcam, bg = TG._set(sc), TG._cam(cam), torch.zeros(3, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    m = torch.rand(sc.P, device=DEV, generator=g) < 0.5
    sub = GaussianSet(pc._xyz[m].detach(), pc._scaling[m].detach(), pc._rotation[m].detach(), pc._opacity[m].detach(),
                      pc._features[m].detach(), pc._semantics[m].detach(), pc.active_sh_degree)
    lab, K = VR.label_map("half-plane", 123, 77, True)
    lab = _labels(lab)
    vs = contrib.frame_votes(tcam, sub, bg, lab, K)
    assert bool(vs.any())
    start = torch.randint(-2 ** 40, 2 ** 40, (sc.P, K), dtype=torch.int64, device=DEV, generator=g)
    got = contrib.frame_votes(tcam, pc, bg, lab, K, gaussian_mask=m, votes=start.clone())
    assert torch.equal(got[~m], start[~m]), "unselected rows must keep their start values"
    assert torch.equal(got[m], start[m] + vs), "selected rows must take the votes of the index-selected sub-model"


def test_frame_votes_runs_the_same_forward():
    from goi_hyperplane_amd import contrib
    d = _dump("ragged-123x77")
    P, W, H = d["frame"][:3]
    lab, K = VR.label_map("checkerboard", W, H, True)
    a = contrib.frame_votes(d["cam"], d["pc"], d["bg"], _labels(lab), K)
    assert torch.equal(a, contrib.votes_buffers(*d["frame"], _labels(lab), K)) and bool(a.any())
    assert np.array_equal(a.cpu().numpy(), VR.scatter(d["contribs"], lab, K, P))


@pytest.mark.parametrize("name", ["ragged-123x77", "stack-40-0.9", "masks-400x300"])
def test_assign_and_lift_against_numpy(name):
    from goi_hyperplane_amd import contrib
    d = _dump(name)
    P, W, H = d["frame"][:3]
    for kind in ("half-plane", "64-distinct"):
        lab, K = VR.label_map(kind, W, H, True)
        v = contrib.votes_buffers(*d["frame"], _labels(lab), K)
        tied = int(torch.argmax(v.sum(1)))  # a manufactured tie between the last class and an earlier one
        row = v[tied].clone()
        v[tied, K - 1] = v[tied, 0] = row.max() + 1
        for mw in (0.0, 0.5, 40.0):
            label, share = contrib.assign(v, mw)
            wl, ws = VR.assign(v.cpu().numpy(), mw)
            assert label.dtype == torch.int64 and share.dtype == torch.float32 and label.is_cuda
            assert np.array_equal(label.cpu().numpy(), wl) and np.array_equal(share.cpu().numpy(), ws), (name, kind, mw)
        assert int(contrib.assign(v)[0][tied]) == 0, "the lowest class wins among equals"
        assert (wl == -1).any() and (VR.assign(v.cpu().numpy())[0] >= 0).any()
        if K == 2:
            for thr, mw in ((0.5, 0.0), (0.0, 0.0), (0.9, 1.0)):
                assert np.array_equal(contrib._lift(v, thr, mw).cpu().numpy(), VR.lift(v.cpu().numpy(), thr, mw))
    # lift_mask, the whole call, for one camera
    mask = torch.from_numpy(VR.label_map("half-plane", W, H)[0].reshape(1, 1, H, W) == 1).to(DEV)
    sel = contrib.lift_mask([d["cam"]], d["pc"], d["bg"], mask, threshold=0.5, min_weight=0.25)
    v2 = VR.scatter(d["contribs"], mask.reshape(-1).cpu().numpy().astype(np.int32), 2, P)
    assert sel.dtype == torch.bool and tuple(sel.shape) == (P,)
    assert np.array_equal(sel.cpu().numpy(), VR.lift(v2, 0.5, 0.25))


def test_lift_mask_on_relevant_cameras_masks():
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.semantic import relevant_cameras
    from tests import test_gpu_relevant_cameras as RC
    dev = torch.device("cuda:0")
    pc, mlp, lut, score_fn = RC._scene(dev)
    cams = RC._cameras(dev)[:6]
    bg = torch.zeros(3, device=dev)
    res = relevant_cameras(cams, pc, mlp, lut, score_fn, 0.5, bg)
    kept = [cams[i] for i in res.index]
    assert len(kept) >= 2 and res.semantic_mask.dtype == torch.bool
    sel = contrib.lift_mask(kept, pc, bg, res.semantic_mask)
    P = int(pc.get_xyz.shape[0])
    assert sel.dtype == torch.bool and tuple(sel.shape) == (P,) and sel.is_cuda
    peak = contrib.peak_weights(kept, pc, bg)
    assert bool(sel.any()) and not bool(sel[peak <= 0].any()), "only Gaussians the kept cameras show can be selected"
    assert int(sel.sum()) < int((peak > 0).sum()), "the masks must leave something out"
