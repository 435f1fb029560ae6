"""tests/trace_reference.py held to account without a GPU:
  * on float32 frames made by blend_reference.cpu_frame it equals a plain per-pixel loop written from the reference's traceCUDA
    (cuda_rasterizer/forward.cu:490-537), ragged images, S = 1, 3, 4;
  * fed the CPU oracle's state after Oracle.trace (its lists and its n_contrib) and float32 direct-form pairs, it reproduces the
    oracle's counts and sums on three small scenes.  numpy's and libm's float32 exp differ by an ulp here and there, so a Gaussian
    is left out iff one of its candidate pairs has a float64 alpha within 1e-5 relative of 0.005 or of 1/255 -- at most 1 % of the
    Gaussians with events, asserted;
  * check_trace can fail: a dropped event, 1 per event instead of S, hits behind n_contrib counted, 1/255 as the threshold, a
    lane outside the image scattering, one ulp on a sum that must be exact, a row that was not cleared.
"""
import math

import numpy as np
import pytest

from tests import blend_reference as BR
from tests import trace_reference as TR


def _frame(seed, W, H, P=60):
    rng = np.random.default_rng(seed)
    m = np.stack([rng.uniform(-2, W + 2, P), rng.uniform(-2, H + 2, P)], 1)
    s1, s2, th = rng.uniform(2, 12, P), rng.uniform(2, 12, P), rng.uniform(0, math.pi, P)
    c_, s_ = np.cos(th), np.sin(th)
    a = c_ * c_ / s1 ** 2 + s_ * s_ / s2 ** 2
    c = s_ * s_ / s1 ** 2 + c_ * c_ / s2 ** 2
    b = c_ * s_ * (1 / s1 ** 2 - 1 / s2 ** 2)
    # a third of the opacities around the two thresholds (1/255 = 0.0039, 0.005), a third large enough to stop pixels early
    o = np.where(np.arange(P) % 3 == 0, rng.uniform(0.003, 0.012, P), np.where(np.arange(P) % 3 == 1, rng.uniform(0.9, 1.0, P),
                                                                                rng.uniform(0.02, 0.5, P)))
    co = np.stack([a, b, c, o], 1)
    # every Gaussian is listed in every tile: the lanes outside a ragged image get their hits too
    return BR.cpu_frame(W, H, m, co, rng.uniform(0, 1, (P, 3)), np.sort(rng.uniform(2, 8, P)), np.zeros((P, 1)), np.zeros(3),
                        dtype=np.float32)


def _images(seed, S, H, W):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (S, H, W)).astype(np.float32), rng.normal(size=(S, H, W)).astype(np.float32)


def _loop(fr, imgs):
    """traceCUDA's pixel loop (forward.cu:490-537) over every pixel of the image, float32 throughout, the sums in float64; one walk
    serves several images.  -> (count [P], n_contrib [HW], [(sum, abs_sum) per image])."""
    f = np.float32
    gx = (fr.W + 15) // 16
    count = np.zeros(fr.P, np.int64)
    sums = [(np.zeros((fr.P, im.shape[0])), np.zeros((fr.P, im.shape[0]))) for im in imgs]
    n_contrib = np.zeros(fr.W * fr.H, np.int64)
    for py in range(fr.H):
        for px in range(fr.W):
            r0, r1 = (int(x) for x in fr.ranges[(py // 16) * gx + px // 16])
            T, contributor, last = f(1), 0, 0
            for k in range(r0, r1):
                contributor += 1
                g = int(fr.point_list[k])
                a, b, c, o = fr.conic_opacity[g]
                dx, dy = fr.means2D[g, 0] - f(px), fr.means2D[g, 1] - f(py)
                power = f(-0.5) * (a * dx * dx + c * dy * dy) - b * dx * dy
                if power > f(0):
                    continue
                alpha = min(f(0.99), o * np.exp(power))
                if alpha < f(1) / f(255):
                    continue
                test_T = T * (f(1) - alpha)
                if test_T < f(0.0001):
                    break  # (done: nothing more happens to this pixel)
                if float(alpha) > 0.005:
                    for im, (tot, mag) in zip(imgs, sums):
                        v = im[:, py, px].astype(np.float64)
                        tot[g] += v
                        mag[g] += np.abs(v)
                    count[g] += 1
                T = test_T
                last = contributor
            n_contrib[py * fr.W + px] = last
    return count, n_contrib, sums


@pytest.mark.parametrize("W,H", [(21, 13), (40, 35)])
def test_reference_equals_the_per_pixel_loop(W, H):
    fr, qd, E, alpha, hit = _frame(7 + W, W, H)
    assert alpha.dtype == np.float32 and fr.means2D.dtype == np.float32
    ref1 = TR.trace_reference(fr, qd, alpha, hit, _images(0, 1, H, W)[1])
    st = ref1.stats
    assert min(st["events"], st["low_alpha_contributors"], st["hits_behind_n_contrib"], st["lanes_outside"], st["hits_outside"]) > 0, st
    imgs = [(img, exact) for S in (1, 3, 4) for img, exact in zip(_images(S, S, H, W), (True, False))]
    count, nc, sums = _loop(fr, [img for img, _ in imgs])
    assert np.array_equal(nc, fr.n_contrib), "the loop's n_contrib is not the frame's"
    for (img, exact), (tot, mag) in zip(imgs, sums):
        ref = TR.trace_reference(fr, qd, alpha, hit, img)
        assert ref.sum.shape == tot.shape and np.array_equal(ref.count, count) and ref.stats["events"] == count.sum()
        if exact:
            assert np.array_equal(ref.sum, tot) and np.array_equal(ref.abs_sum, mag)
        else:  # (two float64 sums of the same terms in two orders)
            assert (np.abs(ref.sum - tot) <= 2.0 ** -50 * count[:, None] * mag).all()
            assert (np.abs(ref.abs_sum - mag) <= 2.0 ** -50 * count[:, None] * mag).all()


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,S,W,H,mu,seed", [(400, 3, 70, 50, -2.4, 11), (600, 4, 123, 77, -2.6, 12), (300, 10, 50, 37, -2.0, 13)])
def test_reference_reproduces_the_oracle(oracle_mod, P, S, W, H, mu, seed):
    from goi_hyperplane_amd.scene import make_camera, make_scene
    sc = make_scene(P, S=S, sh_degree=1, seed=seed, log_scale_mean=mu)
    cam = make_camera(W, H, yaw=0.2, pitch=-0.1)
    img = np.random.default_rng(seed).normal(size=(S, H, W)).astype(np.float32)
    o = oracle_mod.from_scene(sc, cam)
    n, _, gau_sem, num = o.trace(img)
    st = o.state()
    fr = BR.Frame(W, H, S, st["means2D"], st["conic_opacity"], st["rgb"], st["depths"], np.zeros((P, S), np.float32), st["point_list"],
                  st["ranges"], st["n_contrib"], np.zeros(W * H, np.float32), np.zeros(3, np.float32))
    qd = BR.candidates(fr)
    assert qd.npairs > 0 and n == fr.N
    E, alpha, below, seen = BR.direct_pairs(fr, qd, np.float32)
    # (the oracle skips power > 0, direct_pairs power > 1e-4: no pair of these scenes may lie in between)
    m, co, f = fr.means2D[qd.pair_id], fr.conic_opacity[qd.pair_id], np.float32
    dx, dy = m[:, 0:1] - qd.px[qd.pair_quad].astype(f), m[:, 1:2] - qd.py[qd.pair_quad].astype(f)
    power = f(-0.5) * (co[:, 0:1] * dx * dx + co[:, 2:3] * dy * dy) - co[:, 1:2] * dx * dy
    assert power.dtype == f and np.array_equal(below, power <= f(BR.POWER_TOL)) and not (below & (power > 0)).any()
    ref = TR.trace_reference(fr, qd, alpha, below & seen, img)
    a64 = BR.direct_pairs(fr, qd, np.float64)[1]
    near = (np.abs(a64 - 0.005) <= 1e-5 * 0.005) | (np.abs(a64 - 1 / 255) <= 1e-5 / 255)
    out = np.zeros(P, bool)
    out[qd.pair_id[(near & qd.inside[qd.pair_quad]).any(axis=1)]] = True
    has = ref.count > 0
    assert has.sum() > P // 4
    assert (out & has).sum() <= 0.01 * has.sum(), (int((out & has).sum()), int(has.sum()))
    keep = ~out
    assert np.array_equal(num[keep], S * ref.count[keep]), int((num[keep] != S * ref.count[keep]).sum())
    # the oracle adds in double and rounds once: half an ulp of the sum, plus the two double sums' own orders
    tol = BR.U * np.abs(ref.sum) + 2.0 ** -50 * ref.count[:, None] * ref.abs_sum
    assert (np.abs(gau_sem.astype(np.float64) - ref.sum) <= tol)[keep].all()
    print(dict(ref.stats, left_out=int((out & has).sum()), with_events=int(has.sum())))


# ---- check_trace can fail -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    W, H, S = 40, 35, 3
    fr, qd, E, alpha, hit = _frame(47, W, H)
    ints, normal = _images(5, S, H, W)
    return dict(fr=fr, qd=qd, alpha=alpha, hit=hit, S=S, ints=ints, normal=normal,
                ref_i=TR.trace_reference(fr, qd, alpha, hit, ints), ref_n=TR.trace_reference(fr, qd, alpha, hit, normal))


def _result(ref, S):
    """What a correct device leaves: the sums rounded to fp32 (within half an ulp: inside the bound for two or more events, exact
    for one), S per event."""
    return ref.sum.astype(np.float32), (S * ref.count).astype(np.int32)


def _wrong(c, img, **kw):
    """The result of a kernel whose events are `events(**kw)`."""
    count, tot, _ = TR.accumulate(c["fr"], c["qd"], TR.events(c["qd"], c["alpha"], c["hit"], **kw), img)
    return tot.astype(np.float32), (c["S"] * count).astype(np.int32)


def test_a_correct_result_passes(case):
    c = case
    TR.check_trace(c["ref_i"], *_result(c["ref_i"], c["S"]), c["S"], True)
    r = TR.check_trace(c["ref_n"], *_result(c["ref_n"], c["S"]), c["S"], False)
    assert 0 < r["max_ratio"] <= 1
    assert (c["ref_n"].count == 0).any() and (c["ref_n"].count > 64).any()


@pytest.mark.parametrize("exact", [True, False])
def test_a_dropped_event_fails(case, exact):
    c = case
    ref, img = (c["ref_i"], c["ints"]) if exact else (c["ref_n"], c["normal"])
    ev = TR.events(c["qd"], c["alpha"], c["hit"])
    i, lane = np.argwhere(ev)[len(np.argwhere(ev)) // 2]
    pix = c["qd"].pix[c["qd"].pair_quad[i], lane]
    assert img.reshape(c["S"], -1)[:, pix].all(), "the dropped event adds a zero"
    ev[i, lane] = False
    count, tot, _ = TR.accumulate(c["fr"], c["qd"], ev, img)
    with pytest.raises(AssertionError, match="num_gsem"):
        TR.check_trace(ref, tot.astype(np.float32), (c["S"] * count).astype(np.int32), c["S"], exact)
    with pytest.raises(AssertionError, match="gau_sem"):  # (the count right, the sum without it)
        TR.check_trace(ref, tot.astype(np.float32), _result(ref, c["S"])[1], c["S"], exact)


def test_one_per_event_instead_of_S_fails(case):
    c = case
    with pytest.raises(AssertionError, match="num_gsem"):
        TR.check_trace(c["ref_i"], _result(c["ref_i"], c["S"])[0], c["ref_i"].count.astype(np.int32), c["S"], True)


@pytest.mark.parametrize("kw,stat", [(dict(stop=False), "hits_behind_n_contrib"), (dict(threshold=float(BR.ALPHA_MIN32), strict=False),
                                                                                  "low_alpha_contributors"),
                                     (dict(clip=False), "hits_outside")])
def test_a_wrong_event_rule_fails(case, kw, stat):
    c = case
    assert c["ref_i"].stats[stat] > 0
    for ref, img, exact in ((c["ref_i"], c["ints"], True), (c["ref_n"], c["normal"], False)):
        got, num = _wrong(c, img, **kw)
        with pytest.raises(AssertionError, match="num_gsem"):
            TR.check_trace(ref, got, num, c["S"], exact)
        with pytest.raises(AssertionError, match="gau_sem"):  # (even with the counts forged)
            TR.check_trace(ref, got, _result(ref, c["S"])[1], c["S"], exact)


def test_one_ulp_on_an_exact_sum_fails(case):
    c = case
    got, num = _result(c["ref_i"], c["S"])
    g = int(np.argmax(c["ref_i"].count))
    got[g, 1] = np.nextafter(got[g, 1], np.float32(np.inf))
    with pytest.raises(AssertionError, match="must be exactly"):
        TR.check_trace(c["ref_i"], got, num, c["S"], True)


def test_a_row_that_was_not_cleared_fails(case):
    c = case
    for ref, exact in ((c["ref_i"], True), (c["ref_n"], False)):
        got, num = _result(ref, c["S"])
        g = int(np.flatnonzero(ref.count == 0)[0])
        for stale in (np.float32(1e-30), np.float32(-0.0), np.float32(np.nan)):
            bad = got.copy()
            bad[g, 0] = stale
            with pytest.raises(AssertionError, match="without events"):
                TR.check_trace(ref, bad, num, c["S"], exact)
        g = int(np.argmax(ref.count))  # the events added on top of what the row held before
        bad = got.copy()
        bad[g] += np.float32(3.0)
        with pytest.raises(AssertionError, match="gau_sem"):
            TR.check_trace(ref, bad, num, c["S"], exact)
        stale_num = num.copy()
        stale_num[g] += 7
        with pytest.raises(AssertionError, match="num_gsem"):
            TR.check_trace(ref, got, stale_num, c["S"], exact)


def test_check_forward_takes_all_four_maps_or_the_colour_alone(case):
    """A trace has the colour map only; a forward frame that drops or misspells a map is refused, not passed unchecked."""
    fr, qd = case["fr"], case["qd"]
    fw = BR.forward_reference(fr, qd, case["alpha"], case["hit"])
    n = BR.nsem_of(fr.S)
    color = np.zeros((3, fr.W * fr.H), np.float32)
    color[:, qd.pix[qd.inside]] = (fw["acc"][qd.inside][:, n:n + 3] + fw["T"][qd.inside][:, None] * fr.bg[None]).T
    BR.check_forward(fr, qd, fw, dict(color=color), BR.GATE, colour_only=True)
    with pytest.raises(AssertionError, match="maps must hold exactly"):
        BR.check_forward(fr, qd, fw, dict(color=color), BR.GATE)
    with pytest.raises(AssertionError, match="maps must hold exactly"):
        BR.check_forward(fr, qd, fw, dict(color=color, sem=None, depth=None, alpha=None), BR.GATE, colour_only=True)
    with pytest.raises(AssertionError, match="color"):
        BR.check_forward(fr, qd, fw, dict(color=color + np.float32(1e-3)), BR.GATE, colour_only=True)
