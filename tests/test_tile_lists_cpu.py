"""The float64 tile-list reference (tests/tile_list_reference.py) checked against itself on the committed case list
(tests/tile_list_cases.py), and the coverage of that list asserted so the cases cannot rot.  Needs no GPU: everything here comes
from the CPU oracle's forward state and the reference.

Per case: must is a subset of the oracle's list by construction (the classes are arrays over it) and never meets may-not; the
analytic maximum behind may-not agrees with a dense sampling of the grown tile square; a float32 evaluation of `power` in the
reference's operation order accepts no pair classified may-not.  The free band's share (pairs that are neither) is printed per
case -- overall, and on the Gaussians where the ellipse is claimed; docs/MEASUREMENT_LOG.md records the figures."""
import numpy as np
import pytest

from tests import tile_list_cases as cases
from tests import tile_list_reference as ref

SUMMARY = {}
SAMPLE_CAP = 20000  # pairs per case whose analytic maximum is compared with dense sampling (seeded draw beyond that)


def analyse(oracle_mod, name, checks=False):
    if name in SUMMARY and not checks:
        return SUMMARY[name]
    sc, cam = cases.CASES[name]()
    W, H = cam.image_width, cam.image_height
    o = oracle_mod.from_scene(sc, cam, bg=cases.BG)
    f = o.forward()
    st = o.state()
    cl = ref.classify(st, f.radii, W, H)
    g, gid, must, may_not = cl["g"], cl["gid"], cl["must"], cl["may_not"]
    P = cl["P"]
    if checks:
        assert np.isin(cl["keys"][must], cl["keys"]).all()
        assert not (must & may_not).any(), f"{name}: {(must & may_not).sum()} pairs are both must and may-not"
        assert not (must & cl["may_not_box"]).any()
        assert (cl["may_not_box"] <= may_not).all()
        # the analytic maximum against dense sampling
        idx = np.nonzero(g["boxed"][gid])[0]
        if idx.size > SAMPLE_CAP:
            idx = np.sort(np.random.default_rng(1).choice(idx, SAMPLE_CAP, replace=False))
        for s in range(0, idx.size, 4096):
            ii = idx[s:s + 4096]
            smax, slack = ref.sampled_power_max(cl, ii)
            pm = cl["power_max"][ii]
            scale = 1e-9 * (1.0 + np.abs(pm))
            assert (smax <= pm + scale).all(), f"{name}: a sampled point lies above the analytic maximum"
            assert (pm <= smax + slack + scale).all(), f"{name}: the analytic maximum lies above anything nearby"
            # class agreement: wherever the sampling alone decides, it decides as the analytic maximum does
            tau = g["tau_up"][gid[ii]]
            assert not (cl["outside_ellipse"][ii] & (smax >= -tau)).any()
            assert (cl["outside_ellipse"][ii] | ~(smax + slack + scale < -tau)).all()
        # float32, reference operation order: no may-not pair is ever accepted
        mn = np.nonzero(may_not)[0]
        acc = ref.float32_accepts(cl, st, mn)
        assert not acc.any(), f"{name}: float32 accepts {acc.sum()} may-not pairs"
    vis = np.asarray(f.radii) > 0
    has_must = np.zeros(P, bool)
    has_must[gid[must]] = True
    all_may_not = np.ones(P, bool)
    all_may_not[gid[~may_not]] = False
    o32 = g["o32"]
    rob = g["boxed"] & vis & (g["n_box_nom"] == g["n_box_up"])
    for k in range(4):
        rob &= g["box_nom"][k] == g["box_up"][k]
    bx0, bx1, by0, by1 = g["box_up"]
    n_box = np.where(rob, g["n_box_up"], -1)
    single_row = rob & (((by1 - by0 == 1) & (bx1 - bx0 >= 64)) | ((bx1 - bx0 == 1) & (by1 - by0 >= 64)))
    rel = g["det"] / np.maximum(np.maximum(np.abs(g["a"] * g["c"]), g["b"] ** 2), 1e-300)
    # ties: must-pairs that share tile AND depth bits with another must-pair of a non-adjacent id
    dbits = np.asarray(st["depths"], np.float32).view(np.uint32).astype(np.int64)
    mk = np.nonzero(must)[0]
    tkey = cl["tile"][mk] * (1 << 32) + dbits[gid[mk]]
    order = np.lexsort((gid[mk], tkey))
    tk, gg = tkey[order], gid[mk][order]
    same = tk[1:] == tk[:-1]
    tie_pairs = int((same & (gg[1:] - gg[:-1] > 1)).sum())
    grp = {}
    for d, n in zip(*np.unique(dbits[has_must], return_counts=True)):
        if n >= 65:
            ids = np.nonzero(has_must & (dbits == d))[0]
            if (np.diff(ids) > 1).all():
                grp[int(d)] = int(n)
    sides = dict(left=has_must & (g["mx"] < -0.5), right=has_must & (g["mx"] > W - 0.5),
                 top=has_must & (g["my"] < -0.5), bottom=has_must & (g["my"] > H - 0.5))
    claimed = g["ellipse_claimed"][gid] | ~g["opaque_enough"][gid]
    free = ~must & ~may_not
    listed_ids = np.nonzero(has_must)[0]
    unlisted_sure = vis & ~has_must & all_may_not
    s = dict(
        name=name, W=W, H=H, P=P, tiles=cl["gx"] * cl["gy"], pairs=int(cl["keys"].size), must=int(must.sum()),
        may_not=int(may_not.sum()), may_not_box=int(cl["may_not_box"].sum()), free_share=ref.free_share(cl),
        free_share_claimed=float(free[claimed].sum()) / max(int(claimed.sum()), 1), claimed_share=float(claimed.mean()) if claimed.size else 0.0,
        border_only=int(cl["border_only"].sum()),
        o_at_floor=int((vis & (o32 >= ref.F32_INV255) & (o32.astype(np.float64) <= 1.01 / 255.0)).sum()),
        o_one=int((vis & (o32 == np.float32(1.0))).sum()), o_below=int((vis & (o32 < ref.F32_INV255)).sum()),
        det_nonpos=int((vis & (g["det"] <= 0)).sum()), det_tiny=int((vis & (g["det"] > 0) & (rel <= ref.DET_REL)).sum()),
        det_unsafe_listed=int((vis & ~g["det_safe"]).sum()),
        box_counts={int(n): int((n_box == n).sum()) for n in (63, 64, 65, 128, 129)}, box_over_128=int((n_box > 129).sum()),
        single_row_64=int(single_row.sum()), tie_pairs=tie_pairs, tie_groups=len(grp),
        outside={k: int(v.sum()) for k, v in sides.items()},
        visible_unlisted=int(unlisted_sure.sum()),
        listed_exactly=int(has_must.sum()) if bool(((has_must | all_may_not)).all()) else -1,
        interleaved=bool(listed_ids.size and (np.nonzero(~has_must)[0] < listed_ids.max()).any()
                         and (np.nonzero(~has_must)[0] > listed_ids.min()).any() or listed_ids.size == 1 and P > 1),
    )
    SUMMARY[name] = s
    print(f"{name}: pairs {s['pairs']} must {s['must']} may-not {s['may_not']} free {s['free_share']:.4f} "
          f"(where the ellipse is claimed: {s['free_share_claimed']:.4f}, {s['claimed_share']:.2f} of the pairs)")
    return s


@pytest.mark.parametrize("name", list(cases.CASES))
def test_reference_is_consistent_with_itself(oracle_mod, name):
    s = analyse(oracle_mod, name, checks=True)
    assert s["pairs"] > 0 and s["pairs"] <= 2_000_000  # (the numpy reference stays in seconds)
    assert s["must"] > 0


def test_case_list_covers_every_class(oracle_mod):
    S = [analyse(oracle_mod, n) for n in cases.CASES]
    tot = lambda k: sum(s[k] for s in S)  # noqa: E731
    assert tot("may_not") >= 100 and tot("border_only") >= 100
    assert tot("o_at_floor") >= 100 and tot("o_one") >= 100 and tot("o_below") >= 100
    assert tot("det_nonpos") + tot("det_tiny") >= 20 and tot("det_tiny") >= 1
    assert tot("visible_unlisted") >= 100  # visible (radius > 0) and certainly listed nowhere
    for n in (63, 64, 65):
        assert sum(s["box_counts"][n] for s in S) >= 1, n
    assert tot("single_row_64") >= 1
    small = [s for s in S if s["tiles"] <= 2048]
    large = [s for s in S if s["tiles"] > 2048]
    for group in (small, large):
        assert sum(s["box_counts"][128] for s in group) >= 1 and sum(s["box_counts"][129] for s in group) >= 1
        assert sum(s["box_over_128"] for s in group) >= 1
    for side in ("left", "right", "top", "bottom"):
        assert sum(s["outside"][side] for s in S) >= 1, side
    assert tot("tie_groups") >= 1 and tot("tie_pairs") >= 100
    for V in cases.LISTED_COUNTS:
        s = SUMMARY[f"listed_{V}"]
        assert s["listed_exactly"] == V and s["interleaved"] and s["visible_unlisted"] >= 1, (V, s["listed_exactly"])
    # the three large grids select three different emit / ranges paths (binning.hip): 8 832, 12 288 and 32 400 tiles
    assert sorted(s["tiles"] for s in S if s["name"].startswith("grid_")) == [8832, 12288, 32400]
    assert len([n for n in cases.CASES if n.startswith("sweep_")]) >= 40


def test_depth_cut_scene_leaves_nothing_unclassified(oracle_mod):
    """The depth-cut part of the GPU test may skip Gaussians whose determinant the reference calls unsafe: on its scene the
    reference alone leaves none."""
    sc, cam = cases.depth_cut_scene()
    o = oracle_mod.from_scene(sc, cam, bg=cases.BG)
    f = o.forward()
    g = ref.gaussian_terms(o.state())
    vis = np.asarray(f.radii) > 0
    assert vis.sum() > 20_000 and not (vis & ~g["det_safe"]).any()
