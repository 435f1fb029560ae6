"""Every semantic width S = 1..32 end to end: the scene of tests/channel_count_cases.py through the frame kernels at each width,
against the CPU oracle and against the product's own width-32 frame.

The blend and backward kernels are compiled once per S4 = ceil(S / 4) and switch on S % 4, on the parity of S, on the number of
16-column accumulator blocks and on three row widths (tests/test_channel_counts_cpu.py counts the classes); before this module
the suite ran 13 of the 32 widths and never an S4 = 7 instantiation (S = 25..28).

AGAINST THE ORACLE (run_hip, check_forward, check_backward of tests/test_gpu_parity.py; FWD_TOL and BWD_TOL are the project's):
num_rendered, tiles_touched, ranges and point_list equal, n_contrib equal outside the oracle's fragile pixels, the four maps
within FWD_TOL, every gradient within BWD_TOL.

WITHOUT THE ORACLE:
  * the semantic map has exactly S channels and dL_dsemantics exactly S columns: both are handed to the C ABI between NaN guard
    bands, every element inside is written (finite), no element of a band is touched -- a padded channel that leaks, or a row
    stride that is only right for a multiple of 4 or 16, writes beyond the S-th channel or leaves one unwritten;
  * the semantics of width S are the first S columns of the width-32 table, and a channel is an accumulator of its own: channel k
    of the semantic map at width S equals channel k of the width-32 frame BIT FOR BIT, and colour, depth and alpha maps, radii and
    n_contrib are bit-identical at all 32 widths.  The identity holds across S = 16 / 17 as well: the `S >= 16` switch of
    csrc/blend_common.h (poly_coefs) is on the PAIR's quadratic form, not on the channel count, so nothing the forward computes
    per pixel depends on the width; it is asserted against width 32 for every S, not per side.

Each case renders a 460-Gaussian scene at 83 x 69 a few times: well under a second (docs/MEASUREMENT_LOG.md, "Every semantic width
1..32 through the frame kernels").  The oracle's run of a width is computed once per process (channel_count_cases.oracle_reference,
a dict keyed by S, arrays read-only) and used by both tests here and by the CPU module; tests/test_gpu_blend_rows.py needs a
different reference -- float64 rows from the DEVICE's alphas -- and keeps its own per-width frames and rows.
Nothing here is built to make a kernel fault: every frame is a valid forward of the product.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests import channel_count_cases as CC
from tests import raw_frame
from tests.raw_frame import GUARD, ptr
from tests.test_gpu_parity import FWD_TOL, check_backward, check_forward, dev, run_hip  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def frame32(dev):  # noqa: F811
    """the product's width-32 forward: what every narrower frame is compared with, bit for bit"""
    sc, cam = CC.case(32)
    res = run_hip(sc, cam, CC.BG, dev, debug_views=True)
    for a in list(res.values()) + list(res["views"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


@pytest.mark.parametrize("S", CC.WIDTHS)
def test_width_matches_the_oracle_and_the_width_32_frame(dev, frame32, S):  # noqa: F811
    sc, cam = CC.case(S)
    ref = CC.oracle_reference(S)
    f, st = ref["forward"], ref["state"]
    res = run_hip(sc, cam, CC.BG, dev, grads=CC.upstream(S), debug_views=True)
    tag = f"width{S}"
    # ---- against the oracle
    assert res["N"] == f.num_rendered, f"{tag}: num_rendered {res['N']} != {f.num_rendered}"
    v = res["views"]
    assert (v["tiles_touched"].astype(np.uint32) == st["tiles_touched"]).all(), tag
    assert (v["ranges"].astype(np.uint32) == st["ranges"]).all(), tag
    assert (v["point_list"].astype(np.uint32) == st["point_list"]).all(), f"{tag}: sorted instance list differs"
    ok = f.fragile.reshape(-1) == 0
    assert (v["n_contrib"].astype(np.uint32)[ok] == st["n_contrib"][ok]).all(), f"{tag}: n_contrib differs"
    assert res["semantics"].shape == (S, CC.H, CC.W)
    worst = check_forward(res, f, tag)
    g = res["grads"]
    assert g["semantics"].shape == (sc.P, S)
    stats = check_backward(g, ref["grads"], tag)
    print(tag, "forward", worst, "backward", {k: s["max"] for k, s in stats.items()}, flush=True)
    # every column of dL_dsemantics carries a gradient of its own (the upstream maps are independent normal draws)
    assert (np.abs(g["semantics"]).max(axis=0) > 0).all(), f"{tag}: a column of dL_dsemantics is all zero"
    # ---- against the width-32 frame, bit for bit
    assert np.array_equal(_bits(res["semantics"]), _bits(frame32["semantics"][:S])), \
        f"{tag}: channels {np.flatnonzero((_bits(res['semantics']) != _bits(frame32['semantics'][:S])).any(axis=(1, 2))).tolist()} differ from width 32"
    for k in ("render", "depth", "alpha"):
        assert np.array_equal(_bits(res[k]), _bits(frame32[k])), f"{tag}: the {k} map differs from width 32"
    assert np.array_equal(res["radii"], frame32["radii"])
    for k in ("n_contrib", "point_list", "ranges"):
        assert np.array_equal(v[k], frame32["views"][k]), f"{tag}: {k} differs from width 32"
    vis = f.radii > 0
    for k in ("tiles_touched", "means2D", "conic_opacity", "rgb", "depths"):
        assert np.array_equal(v[k][vis], frame32["views"][k][vis]), f"{tag}: {k} differs from width 32"


@pytest.mark.parametrize("S", CC.WIDTHS)
def test_exactly_S_channels_are_written(dev, S):  # noqa: F811
    """The C ABI called raw, the semantic map and dL_dsemantic between NaN guard bands (and NaN inside before the call)."""
    from goi_hyperplane_amd import _lib
    sc, cam = CC.case(S)
    fr = raw_frame.RawFrame(sc, cam, CC.BG, "cuda")
    lib, P, N = fr.lib, fr.P, fr.N
    assert N > 0
    n_map = S * CC.H * CC.W
    gm = fr.semmap_guarded.cpu().numpy()
    assert np.isnan(gm[:GUARD]).all() and np.isnan(gm[GUARD + n_map:]).all(), "the forward wrote outside its S channels"
    assert np.isfinite(gm[GUARD:GUARD + n_map]).all(), "an element of the semantic map was not written"
    ref = CC.oracle_reference(S)
    okpix = ref["forward"].fragile.reshape(-1) == 0
    d = np.abs(gm[GUARD:GUARD + n_map].reshape(S, -1) - ref["forward"].semantic.reshape(S, -1))[:, okpix]
    assert d.max() < FWD_TOL  # (this frame is the default forward, called raw)
    M = sc.shs.shape[1]
    shapes = dict(mean2D=(P, 3), conic=(P, 4), opacity=(P,), color=(P, 3), depth=(P,), mean3D=(P, 3), cov3D=(P, 6), sh=(P, M, 3),
                  scale=(P, 3), rot=(P, 4))
    nan = float("nan")
    g = {k: torch.full(s, nan, device="cuda") for k, s in shapes.items()}
    sem_guarded = torch.full((P * S + 2 * GUARD,), nan, device="cuda")
    g["semantic"] = sem_guarded[GUARD:GUARD + P * S]
    scratch = torch.empty(lib.goi_raster_backward_scratch_bytes(N, S), dtype=torch.uint8, device="cuda")
    ups = [torch.from_numpy(np.ascontiguousarray(u)).to("cuda") for u in CC.upstream(S)]
    r = lib.goi_raster_backward(C.byref(fr.scene), N, 0, 0, ptr(fr.geom), ptr(fr.binning), ptr(fr.img), ptr(fr.radii), ptr(fr.alpha),
                                *[ptr(u) for u in ups],
                                *[ptr(g[k]) for k in ("mean2D", "conic", "opacity", "color", "semantic", "depth", "mean3D", "cov3D", "sh",
                                                      "scale", "rot")], ptr(scratch), None, None, None, None)
    assert r >= 0, _lib.last_error()
    torch.cuda.synchronize()
    sg = sem_guarded.cpu().numpy()
    assert np.isnan(sg[:GUARD]).all() and np.isnan(sg[GUARD + P * S:]).all(), "the backward wrote outside dL_dsemantic's [P, S]"
    got = sg[GUARD:GUARD + P * S].reshape(P, S)
    assert np.isfinite(got).all(), f"columns {np.flatnonzero(~np.isfinite(got).all(axis=0)).tolist()} of dL_dsemantic were not written everywhere"
    check_backward(dict(semantics=got), ref["grads"], "", names=("semantics",))
