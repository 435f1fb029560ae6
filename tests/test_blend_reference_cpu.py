"""tests/blend_reference.py held to account without a GPU:
  * its float64 backward against float64 AUTOGRAD of a compositing function of (mean2D, conic, opacity, features, depth) with the
    contribution decisions held fixed and the 0.99 clamp straight-through, to 1e-10 relative; and against tests/torch_reference.py
    where the two overlap (dL/dopacity, dL/dsemantics, dL/dmean2D of a whole small scene);
  * every checker can fail: a row in a neighbouring slot, a flipped validity byte, a dropped or extra member bit, qcost off by one,
    one element off by twice its tolerance, and rows perturbed by 2^-17 per product (the two-bf16-plane flush that render_bwd.hip's
    header says was replaced), which must trip the median / p99 gate;
  * the two test hooks refuse NULLs, a bad mode and misaligned buffers by name, before anything touches a device.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import blend_reference as BR


def _small_scene(seed, P=24, W=40, H=24, S=3, dtype=np.float64, opaque=False):
    rng = np.random.default_rng(seed)
    m = np.stack([rng.uniform(-2, W + 2, P), rng.uniform(-2, H + 2, P)], 1)
    s1, s2, th = rng.uniform(1.5, 9, P), rng.uniform(1.5, 9, P), rng.uniform(0, math.pi, P)
    c_, s_ = np.cos(th), np.sin(th)
    a = c_ * c_ / s1 ** 2 + s_ * s_ / s2 ** 2
    c = s_ * s_ / s1 ** 2 + c_ * c_ / s2 ** 2
    b = c_ * s_ * (1 / s1 ** 2 - 1 / s2 ** 2)
    o = rng.uniform(0.05, 1.0, P)
    if opaque:  # clamped alphas: opacity above 0.99 and the centre on a pixel
        o, m = rng.uniform(0.992, 1.0, P), np.round(m)
    co = np.stack([a, b, c, o], 1)
    fr, qd, E, alpha, hit = BR.cpu_frame(W, H, m, co, rng.uniform(0, 1, (P, 3)), np.sort(rng.uniform(2, 8, P)), rng.normal(size=(P, S)),
                                         np.array([0.3, 0.7, 0.1]), radius=3 * np.maximum(s1, s2), dtype=dtype)
    up = dict(color=rng.normal(size=(3, H, W)), sem=rng.normal(size=(S, H, W)), depth=rng.normal(size=(H, W)),
              alpha=rng.normal(size=(H, W)))
    if dtype == np.float32:
        up = {k: v.astype(np.float32) for k, v in up.items()}
    return fr, qd, E, alpha, hit, up


def _autograd(fr, qd, hit, up):
    """float64 autograd of sum(maps * upstream) through a compositing function whose contribution decisions are the frame's."""
    dt = torch.float64
    T_ = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=dt)  # noqa: E731
    m, co = T_(fr.means2D).requires_grad_(), T_(fr.conic_opacity).requires_grad_()
    rgb, dep, sem = T_(fr.rgb).requires_grad_(), T_(fr.depths).requires_grad_(), T_(fr.sem).requires_grad_()
    g, qq = torch.tensor(qd.pair_id), torch.tensor(qd.pair_quad)
    dx = m[g, 0:1] - T_(qd.px)[qq]
    dy = m[g, 1:2] - T_(qd.py)[qq]
    power = -0.5 * (co[g, 0:1] * dx * dx + co[g, 2:3] * dy * dy) - co[g, 1:2] * dx * dy
    raw = co[g, 3:4] * torch.exp(power)
    alpha = raw + (torch.clamp(raw, max=float(BR.ALPHA_MAX32)) - raw).detach()
    contrib = torch.tensor(hit & (qd.pair_pos[:, None] < qd.nc[qd.pair_quad]) & qd.inside[qd.pair_quad])
    feat = torch.cat([sem, rgb, dep[:, None]], 1)
    nch = feat.shape[1]
    T = torch.ones(qd.Q, 64, dtype=dt)
    acc = torch.zeros(qd.Q, 64, nch, dtype=dt)
    for pos in range(int(qd.length.max())):
        act = np.flatnonzero(qd.length > pos)
        idx = torch.tensor(qd.off[act] + pos)
        act_t = torch.tensor(act)
        c = contrib[idx]
        a_ = torch.where(c, alpha[idx], torch.zeros_like(alpha[idx]))
        w = a_ * T[act_t]
        acc = acc.index_add(0, act_t, w[:, :, None] * feat[g[idx]][:, None, :])
        Tn = T.clone()
        Tn[act_t] = T[act_t] * (1 - a_)
        T = Tn
    S = fr.S
    pix, ins = torch.tensor(qd.pix), torch.tensor(qd.inside)
    HW = fr.W * fr.H
    gat = lambda a: T_(np.asarray(a).reshape(-1, HW))[:, pix]  # noqa: E731  [C, Q, 64]
    bg = T_(fr.bg)
    loss = (acc[:, :, :S].permute(2, 0, 1) * gat(up["sem"]) * ins).sum()
    loss = loss + ((acc[:, :, S:S + 3].permute(2, 0, 1) + T[None] * bg[:, None, None]) * gat(up["color"]) * ins).sum()
    loss = loss + (acc[:, :, S + 3] * gat(up["depth"])[0] * ins).sum() + ((1 - T) * gat(up["alpha"])[0] * ins).sum()
    loss.backward()
    return dict(mean2D=m.grad.numpy(), conic_opacity=co.grad.numpy(), rgb=rgb.grad.numpy(), depth=dep.grad.numpy(), sem=sem.grad.numpy())


@pytest.mark.parametrize("seed,opaque", [(1, False), (2, False), (3, True)])
def test_float64_reference_matches_float64_autograd(seed, opaque):
    fr, qd, E, alpha, hit, up = _small_scene(seed, opaque=opaque)
    rw = BR.backward_rows(fr, qd, up, E, alpha, hit)
    assert rw.member.sum() > 50
    if opaque:
        assert (E > 0.99).any(), "no clamped alpha in the opaque scene"
    got = BR.per_gaussian_sums(fr, qd, rw)
    g = _autograd(fr, qd, hit, up)
    S, n = fr.S, BR.nsem_of(fr.S)
    want = np.zeros_like(got)
    want[:, :S] = g["sem"]
    want[:, n:n + 3], want[:, n + 3] = g["rgb"], g["depth"]
    want[:, n + 4], want[:, n + 5] = 0.5 * fr.W * g["mean2D"][:, 0], 0.5 * fr.H * g["mean2D"][:, 1]  # NDC units
    want[:, n + 6], want[:, n + 8] = g["conic_opacity"][:, 0], g["conic_opacity"][:, 2]
    want[:, n + 7] = 0.5 * g["conic_opacity"][:, 1]  # (the reference's convention: -1/2 on the off-diagonal element too)
    want[:, n + 9] = g["conic_opacity"][:, 3]
    scale = np.abs(want).max(axis=0)
    assert (np.abs(got - want) <= 1e-10 * scale[None]).all(), float((np.abs(got - want) / np.maximum(scale, 1e-300)[None]).max())
    assert (rw.mag[rw.member] >= np.abs(rw.rows[rw.member]) * (1 - 1e-12)).all(), "a magnitude companion is below its element"


def test_reference_agrees_with_the_dense_torch_reference_where_they_overlap():
    """A whole small scene through tests/torch_reference.py (float64, autograd from the 3D inputs) and through this module (the 2D
    quantities it reports, the same rectangles): dL/dopacity, dL/dsemantics and dL/dmean2D (NDC units) agree."""
    from goi_hyperplane_amd.scene import make_camera, make_scene
    from tests import torch_reference as TR
    from tests.blend_cases import upstream
    sc = make_scene(60, S=4, sh_degree=1, seed=5, log_scale_mean=-2.2)
    cam = make_camera(48, 32)
    W, H = 48, 32
    up, _ = upstream("random", 4, H, W, "torch")
    bg = np.array([0.3, 0.7, 0.1])
    want = TR.float64_gradients(sc, cam, bg, (up["color"], up["sem"], up["depth"][None], up["alpha"][None]), 1)
    T_ = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    with torch.no_grad():
        r = TR.render(T_(sc.means3D), T_(sc.opacities), T_(sc.semantics), T_(cam.world_view_transform), T_(cam.full_proj_transform),
                      T_(cam.camera_center), cam.tanfovx, cam.tanfovy, W, H, T_(bg), shs=T_(sc.shs), sh_degree=1, scales=T_(sc.scales),
                      rotations=T_(sc.rotations))
    m, radii = r["means2D"].numpy(), r["radii"].numpy().astype(np.float64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    t = lambda v, g: np.clip(np.trunc(v / 16), 0, g).astype(np.int64)  # noqa: E731
    rects = np.stack([t(m[:, 0] - radii, gx), t(m[:, 1] - radii, gy), t(m[:, 0] + radii + 15, gx), t(m[:, 1] + radii + 15, gy)], 1)
    rects[radii <= 0] = 0
    hom = np.c_[sc.means3D.astype(np.float64), np.ones(sc.P)] @ cam.world_view_transform.astype(np.float64)
    co = np.c_[r["conic"].numpy(), sc.opacities.astype(np.float64).reshape(-1)]
    fr, qd, E, alpha, hit = BR.cpu_frame(W, H, m, co, r["rgb"].numpy(), hom[:, 2], sc.semantics.astype(np.float64), bg, rects=rects,
                                         dtype=np.float64, alpha_min=1.0 / 255.0)
    np.testing.assert_allclose(1 - fr.extra["T_final"].reshape(H, W), r["alpha"][0].numpy(), atol=1e-12)
    got = BR.per_gaussian_sums(fr, qd, BR.backward_rows(fr, qd, up, E, alpha, hit))
    n = BR.nsem_of(4)
    for name, a, b in (("opacity", got[:, n + 9], want["opacity"].reshape(-1)), ("semantics", got[:, :4], want["semantics"]),
                       ("mean2D", got[:, n + 4:n + 6], want["means2D"][:, :2])):
        assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max(), (name, float(np.abs(a - b).max()), float(np.abs(b).max()))


# ---- every checker can fail -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_like():
    """A float32 frame and what a correct device would leave for it: member words, qcost, aux, validity bytes, a row scratch
    holding the float32 yardstick's rows (NaN elsewhere)."""
    fr, qd, E, alpha, hit, up = _small_scene(7, P=150, W=72, H=40, S=5, dtype=np.float32)
    ref = BR.backward_rows(fr, qd, up, E, alpha, hit)
    y = BR.backward_rows(fr, qd, up, E, alpha, hit, dtype=np.float32)
    member = BR.member_reference(qd, hit)
    assert np.array_equal(member, ref.member) and qd.qmax.max() > 64
    N, P = fr.N, fr.P
    count = np.bincount(fr.point_list.astype(np.int64), minlength=P)
    order = np.random.default_rng(0).permutation(np.flatnonzero(count))
    aux = np.zeros((P, 4), np.uint32)
    aux[:, 0] = N
    aux[order, 0] = np.cumsum(count[order]) - count[order]
    qmask0 = np.zeros(qd.Q, np.uint64)
    qmask = np.zeros(4 * (N // 64 + 2), np.uint64)
    for i in np.flatnonzero(member):
        tq, pos = int(qd.pair_quad[i]), int(qd.pair_pos[i])
        r, bit = pos >> 6, np.uint64(1) << np.uint64(pos & 63)
        if r == 0:
            qmask0[tq] |= bit
        else:
            qmask[4 * ((int(qd.x0[tq]) >> 6) + r) + (tq & 3)] |= bit
    slots = BR.slots_reference(fr, qd, aux)
    flags = np.zeros(4 * N, np.uint8)
    flags[slots[member]] = 1
    rf = BR.row_floats(fr.S)
    scratch = np.full((4 * N, rf), np.nan, np.float32)
    scratch[slots[member], :y.rows.shape[1]] = y.rows[member]
    return dict(fr=fr, qd=qd, E=E, alpha=alpha, hit=hit, up=up, ref=ref, y=y, member=member, aux=aux, qmask0=qmask0, qmask=qmask,
                slots=slots, flags=flags, scratch=scratch)


def _gather(d, scratch):
    ncol = BR.nsem_of(d["fr"].S) + 10
    got = np.zeros((d["qd"].npairs, ncol), np.float32)
    got[d["member"]] = scratch[d["slots"][d["member"]]][:, :ncol]
    return got


def test_a_correct_result_passes_every_checker(device_like):
    d = device_like
    BR.check_masks(d["qd"], d["hit"], d["qmask0"], d["qmask"], d["qd"].qmax.copy())
    BR.check_flags(d["slots"], d["member"], d["flags"], d["fr"].N)
    err = BR.check_rows(d["fr"].S, d["qd"], d["ref"], _gather(d, d["scratch"]), BR.GATE, "clean")
    BR.check_gate(BR.class_stats(d["fr"].S, err), BR.GATE)
    fw = BR.forward_reference(d["fr"], d["qd"], d["alpha"], d["hit"])
    n = BR.nsem_of(d["fr"].S)
    HW = d["fr"].W * d["fr"].H
    maps = dict(sem=np.zeros((d["fr"].S, HW)), color=np.zeros((3, HW)), depth=np.zeros(HW), alpha=np.zeros(HW))
    ins, pix = d["qd"].inside, d["qd"].pix
    for ch in range(d["fr"].S):
        maps["sem"][ch, pix[ins]] = fw["acc"][ins][:, ch]
    for ch in range(3):
        maps["color"][ch, pix[ins]] = fw["acc"][ins][:, n + ch] + fw["T"][ins] * float(d["fr"].bg[ch])
    maps["depth"][pix[ins]] = fw["acc"][ins][:, n + 3]
    maps["alpha"][pix[ins]] = 1 - fw["T"][ins]
    BR.check_forward(d["fr"], d["qd"], fw, maps, BR.GATE)
    maps["depth"][pix[ins][5]] += 1e-3 * (1 + abs(maps["depth"][pix[ins][5]]))
    with pytest.raises(AssertionError, match="depth"):
        BR.check_forward(d["fr"], d["qd"], fw, maps, BR.GATE)


def test_a_row_in_a_neighbouring_slot_fails(device_like):
    d = device_like
    s = int(d["slots"][d["member"]][3])
    scratch, flags = d["scratch"].copy(), d["flags"].copy()
    t = s + 1 if flags[s + 1] == 0 else s - 1
    scratch[t], scratch[s] = scratch[s].copy(), np.nan
    flags[t], flags[s] = 1, 0
    with pytest.raises(AssertionError, match="not written"):
        BR.check_rows(d["fr"].S, d["qd"], d["ref"], _gather(d, scratch), BR.GATE, "moved")
    with pytest.raises(AssertionError, match="validity byte"):
        BR.check_flags(d["slots"], d["member"], flags, d["fr"].N)
    aux = d["aux"].copy()  # a wrong first slot: the partition check of slots_reference
    g = int(d["qd"].pair_id[np.flatnonzero(d["member"])[0]])
    aux[g, 0] += 1
    with pytest.raises(AssertionError, match="partition"):
        BR.slots_reference(d["fr"], d["qd"], aux)


@pytest.mark.parametrize("to", [0, 1, 255])
def test_a_flipped_validity_byte_fails(device_like, to):
    d = device_like
    flags = d["flags"].copy()
    s = int(np.flatnonzero(flags == (0 if to else 1))[11])
    flags[s] = to
    with pytest.raises(AssertionError, match=f"validity byte of slot {s}"):
        BR.check_flags(d["slots"], d["member"], flags, d["fr"].N)


@pytest.mark.parametrize("kind", ["dropped-round0", "dropped-round1", "extra"])
def test_a_dropped_or_extra_member_bit_fails(device_like, kind):
    d = device_like
    qd = d["qd"]
    qmask0, qmask = d["qmask0"].copy(), d["qmask"].copy()
    below = qd.pair_pos < qd.qmax[qd.pair_quad]
    if kind == "extra":
        i = int(np.flatnonzero(~d["member"] & below & (qd.pair_pos < 64))[0])
    else:
        i = int(np.flatnonzero(d["member"] & ((qd.pair_pos >= 64) == (kind == "dropped-round1")))[0])
    tq, pos = int(qd.pair_quad[i]), int(qd.pair_pos[i])
    bit = np.uint64(1) << np.uint64(pos & 63)
    if pos < 64:
        qmask0[tq] ^= bit
    else:
        qmask[4 * ((int(qd.x0[tq]) >> 6) + (pos >> 6)) + (tq & 3)] ^= bit
    with pytest.raises(AssertionError, match=f"member bit of quadrant {tq} position {pos}"):
        BR.check_masks(qd, d["hit"], qmask0, qmask, qd.qmax.copy())
    # bits at and beyond qcost are unspecified: setting one changes nothing
    qmask0, qmask = d["qmask0"].copy(), d["qmask"].copy()
    q = int(np.flatnonzero((qd.qmax < 64) & (qd.qmax > 0))[0])
    qmask0[q] |= np.uint64(1) << np.uint64(int(qd.qmax[q]))
    BR.check_masks(qd, d["hit"], qmask0, qmask, qd.qmax.copy())


@pytest.mark.parametrize("delta", [-1, 1])
def test_qcost_off_by_one_fails(device_like, delta):
    d = device_like
    qcost = d["qd"].qmax.copy()
    q = int(np.flatnonzero(qcost > 1)[2])
    qcost[q] += delta
    with pytest.raises(AssertionError, match=rf"qcost\[{q}\]"):
        BR.check_masks(d["qd"], d["hit"], d["qmask0"], d["qmask"], qcost)


@pytest.mark.parametrize("element", [0, 4, 8, 9, 12, 13, 15, 17])
def test_one_element_off_by_twice_its_tolerance_fails(device_like, element):
    d = device_like
    S = d["fr"].S
    got = _gather(d, d["scratch"]).astype(np.float64)
    tol = BR.element_tolerance(S, d["qd"], d["ref"], BR.GATE)
    i = int(np.flatnonzero(d["member"] & (d["ref"].mag[:, element] > 0))[17])
    got[i, element] = d["ref"].rows[i, element] + 2 * tol[i, element]
    with pytest.raises(AssertionError, match=f"element {element}"):
        BR.check_rows(S, d["qd"], d["ref"], got, BR.GATE, "off")
    got = _gather(d, d["scratch"])
    got[i, 5] = 1e-30  # a padded semantic channel (S = 5: channels 5..7)
    with pytest.raises(AssertionError, match="padded"):
        BR.check_rows(S, d["qd"], d["ref"], got, BR.GATE, "pad")


def test_two_bf16_planes_per_operand_trip_the_gate(device_like):
    """w and h carried to 2^-17 (two bf16 planes, three of the four product terms: what render_bwd.hip's header says was replaced):
    every element may still pass its own tolerance, but the distribution does not pass the median / p99 gate."""
    d = device_like
    S = d["fr"].S
    noisy = BR.backward_rows(d["fr"], d["qd"], d["up"], d["E"], d["alpha"], d["hit"], dtype=np.float32,
                             noise=(np.random.default_rng(1), 2.0 ** -17))
    err, _ = BR.normalised_errors(S, d["ref"], noisy.rows, BR.feature_term(S, d["qd"], d["ref"]))
    st = BR.class_stats(S, err)
    with pytest.raises(AssertionError, match="median|p99"):
        BR.check_gate(st, BR.GATE)
    for c in ("features", "colour_depth", "opacity"):
        assert st[c][0] > 4 * BR.GATE[c][0] or st[c][1] > 4 * BR.GATE[c][1], (c, st[c])


# ---- argument validation of the two hooks ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.goi_raster_last_error().decode()


def test_pair_eval_refuses_bad_arguments(lib):
    p = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
    f = lib.goi_raster_debug_pair_eval
    assert f(0, 16, 16, p, p, 1, p, p, p, None) < 0 and "bad P/W/H" in _err(lib)
    assert f(4, 16, 0, p, p, 1, p, p, p, None) < 0 and "bad P/W/H" in _err(lib)
    assert f(4, 16, 16, p, p, -1, p, p, p, None) < 0 and "n_requests" in _err(lib)
    assert f(4, 16, 16, p, p, 0, None, None, None, None) == 0
    for k in range(5):
        a = [p] * 5
        a[k] = None
        assert f(4, 16, 16, a[0], a[1], 1, a[2], a[3], a[4], None) < 0 and "NULL" in _err(lib)
    assert f(4, 16, 16, C.c_void_p((1 << 20) + 64), p, 1, p, p, p, None) < 0 and "256-byte aligned" in _err(lib)
    assert f(4, 16, 16, p, C.c_void_p((1 << 20) + 4), 1, p, p, p, None) < 0 and "8-byte aligned" in _err(lib)
    assert f(4, 16, 16, p, p, 1, C.c_void_p((1 << 20) + 2), p, p, None) < 0 and "4-byte aligned" in _err(lib)


def test_backward_blend_refuses_bad_arguments(lib):
    from goi_hyperplane_amd._lib import GoiRasterScene
    p = C.c_void_p(1 << 20)
    odd = lambda k: C.c_void_p((1 << 20) + k)  # noqa: E731
    f = lib.goi_raster_debug_backward_blend

    def scene(**kw):
        s = GoiRasterScene()
        s.P, s.S, s.W, s.H, s.bg, s.semantics = 8, 10, 32, 32, 1 << 20, 1 << 20
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def call(sc=None, R=5, mode=0, **kw):
        a = dict(geom=p, binning=p, image=p, radii=p, out_alpha=p, c=p, s=p, d=p, a=p, scratch=p, rows=p, flags=p, aux=p, qmask0=p,
                 qmask=p, qcost=p, qorder=p, m2=p, con=p, op=p, col=p, sem=p, dep=p)
        a.update(kw)
        return f(C.byref(sc if sc is not None else scene()), R, mode, *a.values(), None)

    assert f(None, 5, 0, *[p] * 23, None) < 0 and "scene is NULL" in _err(lib)
    assert call(scene(P=0)) < 0 and "bad P/W/H" in _err(lib)
    assert call(scene(S=33)) < 0 and "1 <= S <= 32" in _err(lib)
    assert call(R=0) < 0 and "R > 0" in _err(lib)
    for mode in (-1, 9, 100):
        assert call(mode=mode) < 0 and "unknown mode" in _err(lib)
    assert call(scene(bg=None)) < 0 and "scene.bg" in _err(lib)
    assert call(scene(S=8, semantics=(1 << 20) + 4)) < 0 and "16-byte aligned" in _err(lib)
    for k in ("geom", "binning", "image"):
        assert call(**{k: None}) < 0 and "workspace pointer is NULL" in _err(lib)
        assert call(**{k: odd(128)}) < 0 and "256-byte aligned" in _err(lib)
    for k in ("radii", "out_alpha"):
        assert call(**{k: None}) < 0 and "radii and out_alpha" in _err(lib)
    assert call(mode=4, s=None) < 0 and "dL_dout_semantic" in _err(lib)
    assert call(scratch=None) < 0 and "need the scratch" in _err(lib)
    assert call(scratch=odd(64)) < 0 and "scratch must be 256-byte aligned" in _err(lib)
    assert call(rows=None) < 0 and "rows and row_flags" in _err(lib)
    assert call(flags=None) < 0 and "rows and row_flags" in _err(lib)
    assert call(rows=odd(4)) < 0 and "rows must be 16-byte aligned" in _err(lib)
    for k in ("m2", "con", "op", "col", "sem", "dep"):
        assert call(mode=8, **{k: None}) < 0 and "six per-id arrays" in _err(lib)
    assert call(aux=odd(8)) < 0 and "aux must be 16-byte aligned" in _err(lib)
    assert call(qmask0=odd(4)) < 0 and "8-byte aligned" in _err(lib)
    assert call(mode=8, qmask=odd(4), scratch=None, rows=None, flags=None) < 0 and "8-byte aligned" in _err(lib)
