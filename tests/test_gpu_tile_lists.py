"""The culled tile lists (cull_variant 1: contribution box, cull_variant 2, the default: ellipse tile masks -- preprocess_fwd.hip
phase B, listed_rect / tile_instance / select_bit in common.h, emit_k / emit_big_k) looked at AS LISTS, against the float64
contribution set of tests/tile_list_reference.py, on the adversarial case list of tests/tile_list_cases.py (whose coverage
tests/test_tile_lists_cpu.py asserts).  Every assertion on a list is exact:

  * cull_variant 0: point_list, ranges, tiles_touched and num_rendered equal the oracle's;
  * cull_variant 1 and 2: every tile's list is the oracle's list of that tile filtered IN ORDER by the set the device lists
    there (no reordering -- ties in depth stay in id order --, no duplicate, no foreign id); ranges are consistent;
    tiles_touched[g] is the number of tiles listing g; their sum is the list's length and the returned count;
  * nesting per tile: list2 within list1 within list0;
  * every must-pair is in list1 and in list2; no may-not pair is in list2, no may-not pair of the box in list1;
  * all outputs are bit-identical between the three variants, and so is every pixel's last contributor (n_contrib is a position
    in the tile's list, so its VALUE depends on the culling; the Gaussian it names does not), gradients equal up to the order of one fp32 sum
    (tests/test_gpu_parity.py::_check_culled; on the needle cases -- tests/tile_list_cases.py::NEEDLE_CASES -- opacity,
    semantics, colour and mean2D are held to it, the geometry gradients only on the rows of Gaussians that are no needles:
    a needle's own geometry gradients measure the conditioning of the covariance chain, not the lists).

The depth-cut part checks the lists of a frame cut at a learnt per-tile depth.  A module fixture writes tile_list_stats.json
(per case: |must|, |list2|, |list1|, |list0|, |may-not|, free share) next to the GPU suite's other artefacts."""
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import tile_list_cases as cases
from tests import tile_list_reference as ref
from tests.test_gpu_parity import _check_culled, dev  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _artefact_dir():
    """Where the GPU suite's artefacts go (parity_stats.json of tests/conftest.py, binding_host_time.json): the repository's one
    ignored `*_out/` scratch directory, taken from .gitignore so that this module and the ignore rule cannot drift apart."""
    with open(os.path.join(ROOT, ".gitignore")) as fh:
        names = [line.strip().rstrip("/") for line in fh if line.strip().endswith("_out/")]
    assert len(names) == 1, names
    return os.path.join(ROOT, names[0])


@pytest.fixture(scope="module")
def stats():
    t0 = time.time()
    table = {}
    yield table
    out = _artefact_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "tile_list_stats.json"), "w") as fh:
        json.dump({"cases": table, "module_wall_seconds": round(time.time() - t0, 1)}, fh, indent=1, sort_keys=True)


def _raw_args(sc, cam, tcam, pc, bg):
    return (bg, pc._xyz.detach(), torch.Tensor([]), pc._semantics.detach(), pc._opacity.detach(), pc._scaling.detach(),
            pc._rotation.detach(), 1.0, torch.Tensor([]), tcam.world_view_transform, tcam.full_proj_transform, cam.tanfovx,
            cam.tanfovy, cam.image_height, cam.image_width, pc._features.detach(), sc.sh_degree, tcam.camera_center, False, False)


def _lists(args, P, W, H):
    """The raw op and its workspaces, as tests.test_gpu_parity.run_hip reaches them."""
    from goi_hyperplane_amd import _C
    n, *_outs, geom, binning, img = _C.rasterize_gaussians(*args)
    v = _C.debug_views(P, W, H, n, geom, binning, img)
    return int(n), {k: v[k].cpu().numpy() for k in ("point_list", "ranges", "tiles_touched", "n_contrib", "depths")}, n


def _check_list(tag, n, v, P, universe):
    """What holds for a culled list whatever it keeps; returns its keys."""
    keys = ref.pair_keys(v["point_list"], v["ranges"], P, tag)  # (checks the ranges)
    assert keys.size == n, f"{tag}: the list holds {keys.size} pairs, the returned count is {n}"
    ref.assert_sublist(universe, keys, tag)
    tt = v["tiles_touched"].astype(np.int64)
    assert (np.bincount(keys % P, minlength=P) == tt).all(), f"{tag}: tiles_touched is not the number of tiles listing a Gaussian"
    assert int(tt.sum()) == n, f"{tag}: sum of tiles_touched {int(tt.sum())} != {n}"
    return keys


def _check_culled_needle_case(ref_, culled, sc, tag):
    """_check_culled for a case built with needles (tests/tile_list_cases.py::NEEDLE_CASES has the reasoning): outputs bit-identical;
    opacity and semantics -- which do not pass through the cancelling covariance chain -- within 1e-5 of scale, colour within
    1e-3 and mean2D within 2e-5 as in _check_culled; the geometry gradients within 1e-3 of scale on the rows of every Gaussian
    whose aspect ratio is at most NEEDLE_ASPECT."""
    (n0, o0, g0, v0), (n1, o1, g1, v1) = ref_, culled
    assert n1 < n0, (tag, n0, n1)
    for k in o0:
        assert torch.equal(o0[k], o1[k]), (tag, k)
    round_ = torch.tensor(sc.scales.max(axis=1) / sc.scales.min(axis=1) <= cases.NEEDLE_ASPECT, device=v0.device)
    for k in g0:
        scale = float(g0[k].abs().max())
        d = (g0[k] - g1[k]).abs().reshape(sc.P, -1).amax(dim=1)
        assert torch.isfinite(g1[k]).all(), (tag, k)
        if k in ("_semantics", "_opacity"):
            assert float(d.max()) <= 1e-5 * scale, (tag, k, float(d.max()) / scale)
        elif k == "_features":
            assert float(d.max()) <= 1e-3 * scale, (tag, k, float(d.max()) / scale)
        elif bool(round_.any()):
            assert float(d[round_].max()) <= 1e-3 * scale, (tag, k, float(d[round_].max()) / scale)
    assert float((v0 - v1).abs().max()) <= 2e-5 * float(v0.abs().max()), tag


def _last_contributor(v, W, H):
    """n_contrib of a pixel is a POSITION: how far into its tile's list the pixel's last contributor sits (the reference's
    last_contributor), so its value depends on what else the list holds.  What must not depend on the culling is WHO that is:
    the Gaussian id at that position, -1 where nothing contributed."""
    gx = (W + ref.TILE - 1) // ref.TILE
    y, x = np.divmod(np.arange(W * H, dtype=np.int64), W)
    tile = (y // ref.TILE) * gx + x // ref.TILE
    r = v["ranges"].astype(np.int64).reshape(-1, 2)
    n = v["n_contrib"].astype(np.int64).reshape(-1)
    assert (n >= 0).all() and (n <= (r[:, 1] - r[:, 0])[tile]).all(), "n_contrib points beyond its tile's list"
    pl = v["point_list"].astype(np.int64)
    return np.where(n > 0, pl[np.minimum(r[tile, 0] + n - 1, max(pl.size - 1, 0))] if pl.size else -1, -1)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_tile_lists_against_the_float64_contribution_set(oracle_mod, dev, stats, name):  # noqa: F811
    from goi_hyperplane_amd import _lib
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera, render
    sc, cam = cases.CASES[name]()
    W, H, P, S = cam.image_width, cam.image_height, sc.P, sc.S
    o = oracle_mod.from_scene(sc, cam, bg=cases.BG)
    f = o.forward()
    st = o.state()
    cl = ref.classify(st, f.radii, W, H)
    universe, must, may_not, may_not_box = cl["keys"], cl["must"], cl["may_not"], cl["may_not_box"]

    pc = GaussianSet.from_scene(sc, dev)
    tcam = TorchCamera(cam, dev)
    bg = torch.tensor(cases.BG, device=dev)
    args = _raw_args(sc, cam, tcam, pc, bg)
    gen = torch.Generator(device=dev).manual_seed(2)
    ups = [torch.randn(shape, device=dev, generator=gen) for shape in ((3, H, W), (S, H, W), (1, H, W), (1, H, W))]
    got, keys, ncon = {}, {}, {}
    try:
        for variant in (0, 1, 2):
            _lib.set_option("cull_variant", variant)
            for p in pc.parameters():
                p.grad = None
            out = render(tcam, pc, PipelineParams(), bg)
            torch.autograd.backward((out["render"], out["semantics"], out["depth"], out["alpha"]), ups)
            n, v, _ = _lists(args, P, W, H)
            tag = f"{name}/cull_variant {variant}"
            if variant == 0:
                assert n == f.num_rendered == st["N"], tag
                assert (v["tiles_touched"].astype(np.uint32) == st["tiles_touched"]).all(), tag
                assert (v["ranges"].astype(np.uint32) == st["ranges"]).all(), tag
                assert (v["point_list"].astype(np.uint32) == st["point_list"]).all(), tag
            keys[variant] = _check_list(tag, n, v, P, universe)
            ncon[variant] = _last_contributor(v, W, H)
            got[variant] = (n, {k: out[k].detach().clone() for k in ("render", "semantics", "depth", "alpha", "radii")},
                            {k: p.grad.clone() for k, p in pc.named_parameters()}, out["viewspace_points"].grad.clone())
    finally:
        _lib.set_option("cull_variant", 2)

    in1, in2 = np.isin(universe, keys[1]), np.isin(universe, keys[2])
    stats[name] = dict(must=int(must.sum()), list2=int(keys[2].size), list1=int(keys[1].size), list0=int(keys[0].size),
                       may_not=int(may_not.sum()), may_not_box=int(may_not_box.sum()), free_share=round(ref.free_share(cl), 5),
                       free_listed2=int((in2 & ~must).sum()), W=W, H=H, P=P)
    print(name, stats[name])
    assert np.array_equal(keys[0], universe)
    assert np.isin(keys[2], keys[1]).all(), f"{name}: list2 is not within list1"
    gid, tile = cl["gid"], cl["tile"]
    for variant, inside in ((1, in1), (2, in2)):
        miss = must & ~inside
        assert not miss.any(), (f"{name}: cull_variant {variant} drops {int(miss.sum())} must-pairs, first (tile, Gaussian) = "
                                f"({int(tile[miss][0])}, {int(gid[miss][0])})")
    bad = may_not_box & in1
    assert not bad.any(), f"{name}: cull_variant 1 lists {int(bad.sum())} pairs outside the box, first Gaussian {int(gid[bad][0]) if bad.any() else -1}"
    bad = may_not & in2
    assert not bad.any(), (f"{name}: cull_variant 2 lists {int(bad.sum())} may-not pairs (lost culling), first (tile, Gaussian) = "
                           f"({int(tile[bad][0]) if bad.any() else -1}, {int(gid[bad][0]) if bad.any() else -1})")
    for variant in (1, 2):
        assert np.array_equal(ncon[0], ncon[variant]), f"{name}: n_contrib names another last contributor at cull_variant {variant}"
        if name in cases.NEEDLE_CASES:
            _check_culled_needle_case(got[0], got[variant], sc, f"{name}/cull_variant {variant}")
        else:
            _check_culled(got[0], got[variant])


def test_depth_cut_lists_drop_exactly_what_lies_behind_the_cut(oracle_mod, dev, stats):  # noqa: F811
    """set_forward_mode(depth_cut=True): a speculative frame of a camera that was rendered before lists, per tile, nothing deeper
    than the depth the previous frame learnt.  Its lists are order-preserving sub-lists of the default lists; a pair is missing
    only if depths[g] > zcut[tile]; and every such pair IS missing for Gaussians that have a tile mask (cull_variant 1 rectangle
    of at most 64 tiles, float64 box safely finite)."""
    from goi_hyperplane_amd import _C, _lib
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    sc, cam = cases.depth_cut_scene()
    W, H, P = cam.image_width, cam.image_height, sc.P
    o = oracle_mod.from_scene(sc, cam, bg=cases.BG)
    f = o.forward()
    st = o.state()
    g = ref.gaussian_terms(st)
    pc = GaussianSet.from_scene(sc, dev)
    tcam = TorchCamera(cam, dev)  # ONE camera object: the cut is keyed by the identity of its tensors
    args = _raw_args(sc, cam, tcam, pc, torch.tensor(cases.BG, device=dev))
    _C.poll_counts(wait=True)
    _C._SPEC.clear()
    _C.forget_depth_cuts()
    try:
        _lib.set_option("cull_variant", 1)
        n1, v1, _ = _lists(args, P, W, H)
        _lib.set_option("cull_variant", 2)
        _C._SPEC.clear()
        _C.set_forward_mode(speculative=True, depth_cut=False)
        for _ in range(4):  # three exact frames teach the capacity policy; the fourth is speculative
            n2, v2, _ = _lists(args, P, W, H)
        assert (v2["depths"][f.radii > 0] == st["depths"][f.radii > 0]).all()
        _C.set_forward_mode(depth_cut=True)
        nl, _vl, lazy_l = _lists(args, P, W, H)  # learns (speculative, uncut)
        assert isinstance(lazy_l, _C.LazyCount) and lazy_l.cut_key is None and lazy_l.cam_key is not None and nl == n2
        torch.cuda.synchronize()
        zcut = _C._DEPTH_CUTS["entries"][lazy_l.cam_key]["z"].clone().cpu().numpy()
        nc, vc, lazy_c = _lists(args, P, W, H)  # the cut frame
        assert lazy_c.cut_key is not None and not lazy_c.cut_failed and not lazy_c.redone and not lazy_c.overflowed
    finally:
        _lib.set_option("cull_variant", 2)
        _C.poll_counts(wait=True)
        _C.set_forward_mode(speculative=True, headroom=2.0, capacity=None, on_overflow="warn", max_ahead=64,
                            inference_speculative=False, min_history=3, depth_cut=False)
        _C.forget_depth_cuts()
    universe = ref.pair_keys(st["point_list"], st["ranges"], P, "oracle")
    k1 = _check_list("depth cut/cull_variant 1", n1, v1, P, universe)
    k2 = _check_list("depth cut/default", n2, v2, P, universe)
    kc = _check_list("depth cut/cut frame", nc, vc, P, k2)  # an order-preserving sub-list of the DEFAULT list
    assert np.isfinite(zcut).any() and kc.size < k2.size, "the frame learnt no cut"
    depths = st["depths"]
    kept = np.isin(k2, kc)
    t, gi = k2 // P, k2 % P
    behind = depths[gi] > zcut[t]
    assert behind[~kept].all(), f"{int((~behind[~kept]).sum())} pairs in front of their tile's cut are missing"
    tt1 = v1["tiles_touched"].astype(np.int64)
    listed = np.bincount(k2 % P, minlength=P) > 0
    skipped = listed & ~g["boxed"]
    assert skipped.sum() <= 0.01 * listed.sum()
    masked = (tt1[gi] <= ref.MASK_TILES) & g["boxed"][gi]
    stay = kept & behind & masked
    assert not stay.any(), f"{int(stay.sum())} pairs behind their tile's cut are still listed, first Gaussian {int(gi[stay][0]) if stay.any() else -1}"
    expected = ref.expected_cut_keys(k2, P, depths, zcut)  # what the cut must keep at the least ...
    assert np.isin(expected, kc).all()
    if not (kept & behind).any():                          # ... and, where every Gaussian has a mask, exactly
        assert np.array_equal(expected, kc)
    stats["depth_cut"] = dict(list1=int(k1.size), list2=int(k2.size), cut=int(kc.size), behind=int(behind.sum()),
                              behind_kept_unmasked=int((kept & behind).sum()), skipped=int(skipped.sum()))
    print("depth_cut", stats["depth_cut"])
