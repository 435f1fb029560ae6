"""tests/channel_count_cases.py on the CPU: the scene reaches what the sweep over S = 1..32 relies on, and the sweep covers every
class the frame kernels dispatch on.

SCENE, from the oracle's forward state (the reference's lists: every tile of a Gaussian's 3-sigma rectangle; the product's
default lists are subsets that hold every contributor, so "short" and "contributors beyond position 64" carry over): an image
that is no multiple of the tile in either direction on at most 6 x 5 tiles, a list longer than 64 entries with a pixel whose
LAST CONTRIBUTOR lies beyond position 64 (the second staging round of the blend, member masks of rounds >= 1), a tile with 1..7
entries, a Gaussian listed in 4 tiles or more, a pixel that saturates and stops early (the float64 composite of
tests/blend_reference.py on the oracle's records and last contributors: a later hit whose product T (1 - alpha) is below 1e-4), a
pixel nobody contributes to, quadrants partly and wholly outside the image.

COVERAGE.  The dispatch rules are restated in tests/channel_count_cases.py and checked here three ways: against the library's own
host function goi_raster_debug_reduce_row_floats for every width, against the rules' expressions in the sources with the number of
sites that test S % 4 and the parity of S in each file (a changed rule or a new site fails this test instead of silently shrinking
the sweep), and then the sweep's widths are counted per class.  The issue that asked for this module names an `S >= 16` switch of the pair polynomial (csrc/blend_common.h, poly_coefs): that S is the pair's
own quadratic a Dx^2 + 2 |b Dx Dy| + c Dy^2, not the channel count -- what DOES change between 16 and 17 channels is the number of
16-column accumulator blocks NB.  Both are covered: widths of either NB, and pairs of the scene on either side of the polynomial's
switch (the scene test).
"""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from tests import blend_reference as BR
from tests import channel_count_cases as CC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "goi_hyperplane_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def ref16():
    return CC.oracle_reference(16)


def test_scene_reaches_every_blend_situation(ref16):
    f, st = ref16["forward"], ref16["state"]
    W, H = CC.W, CC.H
    assert W % 16 and H % 16 and W % 8 and H % 8, "ragged tiles AND ragged quadrants"
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert gx <= 6 and gy <= 5 and st["T"] == gx * gy
    length = (st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]).reshape(gy, gx)
    nc = st["n_contrib"].reshape(H, W).astype(np.int64)
    assert length.max() > 64 and nc.max() > 64, "no second staging round"
    assert (nc > 128).any(), "no third staging round"
    assert ((length >= 1) & (length < 8)).any(), "no tile with fewer than 8 entries"
    assert st["tiles_touched"].max() >= 4
    assert (nc == 0).any() and (f.alpha.reshape(H, W)[nc == 0] == 0).all(), "no pixel without a contributor"
    assert f.fragile.mean() < 0.02
    sc, _cam = CC.case(16)
    fr = BR.Frame(W, H, 16, st["means2D"], st["conic_opacity"], st["rgb"], st["depths"], sc.semantics, st["point_list"], st["ranges"],
                  st["n_contrib"], f.alpha.reshape(-1), CC.BG)
    qd = BR.candidates(fr)
    _E, al, below, seen = BR.direct_pairs(fr, qd)
    fw = BR.forward_reference(fr, qd, al, below & seen)
    with np.errstate(invalid="ignore"):
        saturated = qd.inside & (fw["stop"] < BR.T_MIN)
    assert saturated.sum() >= 10, "no pixel saturates and stops early"
    assert (saturated & (qd.nc < qd.length[:, None])).any()
    outside = ~qd.inside
    assert outside.all(axis=1).any() and (outside.any(axis=1) & ~outside.all(axis=1)).any()
    wide = BR.poly64(fr, qd)["S"] >= BR.WIDE_S
    assert wide.any() and (~wide).any(), "pairs on one side of the pair polynomial's fp64 switch only"


def test_geometry_and_lists_do_not_depend_on_the_width(ref16):
    sc32, _ = CC.case(32)
    for S in (1, 27, 32):
        sc, _cam = CC.case(S)
        assert sc.S == S and sc.semantics.shape == (sc.P, S) and sc.semantics.flags["C_CONTIGUOUS"]
        assert np.array_equal(sc.semantics, sc32.semantics[:, :S])
        r = CC.oracle_reference(S)
        for k in ("point_list", "ranges", "n_contrib", "tiles_touched"):
            assert np.array_equal(r["state"][k], ref16["state"][k]), (S, k)
        assert r["forward"].num_rendered == ref16["forward"].num_rendered
        assert np.array_equal(CC.upstream(S)[1], CC.upstream(32)[1][:S])
    with pytest.raises(ValueError):
        CC.case(0)
    with pytest.raises(ValueError):
        CC.case(33)


def _expr(text):
    return re.sub(r"\s+", "", text)


def _count(name, pattern):
    return len(re.findall(pattern, _src(name)))


def test_restated_dispatch_rules_match_the_sources():
    """The EXPRESSIONS of the rules, whitespace aside, and how many sites of each file test `S & 3` / `S & 1`: a new or a removed
    site fails here and is then given its widths.  (The row widths themselves are checked against the library below.)"""
    common, blend = _src("common.h"), _src("blend_common.h")
    m = re.search(r"inline\s+int\s+bwd_row_floats\(int S\)\s*\{\s*return\s*(.*?);", common, re.S)
    assert m and _expr(m.group(1)) == "((4*((S+3)/4)+4+6+15)/16)*16"
    m = re.search(r"inline\s+int\s+bwd_sem_row_floats\(int S\)\s*\{\s*return\s*(.*?);", common, re.S)
    assert m and _expr(m.group(1)) == "((4*((S+3)/4)+15)/16)*16"
    m = re.search(r"#define GOI_DISPATCH_S4\(S, CALL\)(.*?)\n\n", blend, re.S)
    assert m and "switch(((S)+3)/4)" in _expr(m.group(1))
    arms = re.findall(r"(case (\d)|default):\s*CALL\((\d)\)", m.group(1))
    assert [(a[1], a[2]) for a in arms] == [(str(i), str(i)) for i in range(1, 8)] + [("", "8")], "an S4 class lost its own instantiation"
    m = re.search(r"#define\s+GOI_BWD_LAUNCH_BOUNDS\s+__launch_bounds__\((.*)\)\s*$", _src("render_bwd.hip"), re.M)
    assert m and _expr(m.group(1)) == "64,(S4<=4?GOI_BWD_WAVES:2)"
    mod4, even = r"\(\s*(?:ra\.)?S\s*&\s*3\s*\)\s*==\s*0", r"\(\s*(?:ra\.)?S\s*&\s*1\s*\)\s*==\s*0"
    sites = {name: (_count(name, mod4), _count(name, even)) for name in ("render_fwd.hip", "render_bwd.hip", "render_bwd_sem.hip",
                                                                          "render_bwd_tile.hip", "reduce_rows.hip", "preprocess_bwd.hip")}
    assert sites == {"render_fwd.hip": (1, 0), "render_bwd.hip": (1, 0), "render_bwd_sem.hip": (0, 0), "render_bwd_tile.hip": (1, 0),
                     "reduce_rows.hip": (1, 0), "preprocess_bwd.hip": (1, 1)}, sites
    assert re.search(r"bwd_records\s*==\s*2\s*&&\s*bwd_row_floats\(sc\.S\)\s*==\s*32", _src("api.hip"))
    assert re.search(r"sc->S\s*<\s*1\s*\|\|\s*sc->S\s*>\s*32", _src("api.hip")), "validate() no longer admits exactly S = 1..32"
    for S in CC.WIDTHS:  # the helper modules of the other direct tests restate the same widths
        assert CC.nsem_of(S) == BR.nsem_of(S) and CC.bwd_row_floats(S) == BR.row_floats(S) and CC.bwd_sem_row_floats(S) == BR.sem_row_floats(S)


def test_restated_row_widths_match_the_library():
    from goi_hyperplane_amd import _lib
    lib = _lib.load()
    for S in CC.WIDTHS:
        assert lib.goi_raster_debug_reduce_row_floats(0, S) == CC.bwd_row_floats(S)
        assert lib.goi_raster_debug_reduce_row_floats(1, S) == CC.bwd_row_floats(S)
        assert lib.goi_raster_debug_reduce_row_floats(3, S) == CC.bwd_sem_row_floats(S)
        assert (lib.goi_raster_debug_reduce_row_floats(2, S) > 0) == (CC.bwd_row_floats(S) == 32) == (5 <= S <= 20)


def _classes(widths, key):
    return {CC.dispatch_class(S)[key] for S in widths}


def test_the_sweep_covers_every_dispatch_class():
    assert CC.WIDTHS == tuple(range(1, 33))
    assert _classes(CC.WIDTHS, "S4") == set(range(1, 9))
    assert _classes(CC.WIDTHS, "mod4") == {0, 1, 2, 3}
    assert _classes(CC.WIDTHS, "even") == {True, False}
    assert _classes(CC.WIDTHS, "NB") == {1, 2}
    assert _classes(CC.WIDTHS, "wide_launch_bounds") == {True, False}
    assert _classes(CC.WIDTHS, "row_floats") == {16, 32, 48}
    assert _classes(CC.WIDTHS, "sem_row_floats") == {16, 32}
    assert _classes(CC.WIDTHS, "rows_in_preprocess") == {True, False}
    # every (S4, 16-byte rows or not) pair, on the full sweep and on the paired subset the other forms of the kernels run on
    want = {(s4, v) for s4 in range(1, 9) for v in (True, False)}
    for widths in (CC.WIDTHS, CC.PAIRED_WIDTHS):
        assert {(CC.s4_of(S), S % 4 == 0) for S in widths} == want
    assert len(CC.PAIRED_WIDTHS) == 16 and {27, 28} <= set(CC.PAIRED_WIDTHS)
    for key, vals in (("row_floats", {16, 32, 48}), ("sem_row_floats", {16, 32}), ("NB", {1, 2}), ("even", {True, False})):
        assert _classes(CC.PAIRED_WIDTHS, key) == vals
    # the widths whose S4 = 7 instantiations no other module runs
    assert [S for S in CC.WIDTHS if CC.s4_of(S) == 7] == [25, 26, 27, 28]
