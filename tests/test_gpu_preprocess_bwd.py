"""The per-Gaussian backward kernel (csrc/preprocess_bwd.hip: preprocess_bwd_k) called directly, against the oracle's fp32
chain, bit for bit.

goi_raster_debug_preprocess_backward (include/goi_raster.h) runs the product's own launch_preprocess_bwd on buffers built
here: the scene, which Gaussians are visible, their clamp masks and the blend gradients are the test's choice, nothing
comes from a forward pass of the product.  Every output buffer starts as NaN (a known array under `accumulate`): an
element nobody writes is caught, an element that must not be written is seen to be untouched.

ARITHMETIC.  Every output of every visible Gaussian must be bit-equal to goi_oracle_preprocess_backward (plain build).  Both
are compiled without contraction, spell the same statement sequence and use nothing beyond sqrtf and division; the forward
half of the same translation unit is asserted bit-equal to the oracle by tests/test_gpu_parity.py.  The oracle's chain is
itself held against float64 autograd by tests/test_preprocess_bwd_cpu.py.

CONTROL FLOW.  Persistent workgroups walk 256-id segments, classify ids by ballot (visible / needs zeros / keep), carry a
pending list across segments and drain it in tiles of 224 rows (208 when the kernel sums the rows itself).  With the product's
grid a workgroup takes a second segment only above 3 x 256 x CUs Gaussians; `max_blocks` = 1 .. 3 makes a few thousand
Gaussians walk that path.  The three sources of the blend gradients (per-id arrays, records, rows summed in the kernel) times
with / without dL/dSH are the kernel's six instantiations; the records and rows are laid out with
tests/reduce_rows_reference.py, whose fp32 replay predicts a Gaussian's row sum bit for bit.

Visible Gaussians always lie in front of the near plane and have finite inputs; nothing here is built to make the kernel
fault.
"""
from __future__ import annotations

import ctypes as C
import zlib
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

from tests import preprocess_reference as PR
from tests import reduce_rows_reference as R

pytestmark = pytest.mark.gpu

K = R.kernel_constants()
NAN = float("nan")
SEEN = set()  # (with dL/dSH, source) instantiations launched by this module


def _L():
    from goi_hyperplane_amd import _lib as L
    return L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _seed(tag: str) -> int:
    return zlib.crc32(tag.encode())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scaled(rng, shape):
    """Normal values, each row scaled by 10^k, k = -3 .. 1."""
    return (rng.normal(size=shape) * 10.0 ** rng.integers(-3, 2, size=(shape[0], 1))).astype(np.float32)


# ---- one call ---------------------------------------------------------------------------------------------------------------
@dataclass
class Spec:
    inp: dict                 # PR.make_inputs
    radii: np.ndarray         # int32 [P]: > 0 visible (the caller's choice)
    mask: np.ndarray          # uint8 [P] clamp bits
    cov3D: np.ndarray         # float32 [P,6]
    tag: str
    source: int = 0
    S: int = 4
    dsh: bool = True          # dL_dsh is passed (False with SH colours: factored mode)
    sh: bool = True           # SH colours (False: colors_precomp, no SH path)
    cov_precomp: bool = False  # no scale / rotation path
    prev_radii: np.ndarray | None = None
    overflow: int = 0
    accumulate: bool = False
    max_blocks: int = 0
    listed: float = 0.8       # sources 1, 2: fraction of the Gaussians that are listed (own a record / rows)
    big: tuple = ()           # source 2: instance counts given to the first few listed VISIBLE Gaussians
    dense: bool = False       # source 2: a frame with more than DENSE_RATIO instances per listed Gaussian
    extra: dict = field(default_factory=dict)


def _blend_gradients(sp: Spec, rng):
    """(per-id arrays the chain effectively sees, host buffers of the source).  Sources 1 / 2: a frame laid out as the
    reduction's (tests/reduce_rows_reference.py); a listed Gaussian's values are its record / the fp32 replay of its rows,
    everyone else's are zeros."""
    P, S = sp.inp["P"], sp.S
    up = sp.inp["up"]
    if sp.source == 0:
        return dict(mean2D=up["mean2D"], conic=up["conic"], color=up["color"], depth=up["depth"]), {}
    rf = R.row_floats(sp.source, S)
    vis = np.flatnonzero(sp.radii > 0)
    is_listed = rng.random(P) < sp.listed
    if P < 8:
        is_listed[:] = True
    ids = np.flatnonzero(is_listed)
    rng.shuffle(ids)  # depth order is unrelated to the id
    if sp.big:
        head = [g for g in vis if is_listed[g]][:len(sp.big)]
        ids = np.concatenate([np.asarray(head, dtype=ids.dtype), ids[~np.isin(ids, head)]])
    V = len(ids)
    if sp.source == 1:
        counts = rng.integers(1, 3, V).astype(np.int64)
    else:
        counts = rng.geometric(0.05 if sp.dense else 0.15, V).astype(np.int64)
        counts[:len(sp.big)] = sp.big[:V]
    offsets = np.zeros(V, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)[:-1]
    total = int(counts.sum())
    n_cap = total + 1  # (one spare instance: where the aux word of an unlisted Gaussian points; its rows hold NaN)
    tiles = np.zeros(P, dtype=np.uint32)
    tiles[ids] = counts
    flags = np.where(rng.random(4 * n_cap) < 0.4, rng.integers(1, 256, 4 * n_cap), 0).astype(np.uint8)
    flags[4 * total:] = 255
    fr = R.Frame(P, S, n_cap, total, ids.astype(np.uint32), offsets.astype(np.uint32), tiles, flags, sp.overflow)
    fr_ref = R.Frame(P, S, n_cap, total, fr.order, fr.offsets, tiles, flags, 0)  # (the layout does not depend on the overflow word)
    ref = R.frame_reference(fr_ref, K)
    rows = np.full((4 * n_cap, rf), NAN, dtype=np.float32)
    emap, _ = R.element_map(S, sp.source, rf)
    used = np.array([m is not None for m in emap])
    if sp.source == 1:
        sums = np.full((V, rf), NAN, dtype=np.float32)
        sums[:, used] = _scaled(rng, (V, int(used.sum())))
        rows[R.record_slots(ref, np.arange(V))] = sums
    else:
        vals = _scaled(rng, (len(ref.slots), rf))
        vals[:, ~used] = NAN
        exp = R.expected_sums(ref, vals)
        rows[ref.slots] = vals
        sums = exp.plain.copy()
        big = np.flatnonzero(ref.big)
        assert len(big) == sum(1 for c in sp.big if c > ref.big_inst), (ref.big_inst, sp.big)
        for r in big:  # a big Gaussian: nothing but the record reduce_big_k leaves over its first slot is read
            lo = 4 * int(ref.off0[r])
            rows[lo:lo + 4 * int(counts[r])] = NAN
            sums[r, used] = _scaled(rng, (1, int(used.sum())))[0]
            rows[lo] = sums[r]
        sp.extra.update(big_inst=ref.big_inst, n_big=len(big), rows_summed=int(ref.length.max()) if V else 0)
    widths = R.array_widths(S)
    eff = {n: np.zeros((P, w), dtype=np.float32) for n, w in widths.items()}
    for el, m in enumerate(emap):
        if m is not None:
            eff[m[0]][ids, m[1]] = sums[:, el]
    eff["depth"], eff["opacity"] = eff["depth"].reshape(-1), eff["opacity"].reshape(-1)
    aux = np.zeros((P, 4), dtype=np.uint32)
    aux[:, 0] = total
    aux[ids, 0] = offsets
    aux[:, 1:] = 0xDEAD
    sp.extra["listed"] = is_listed
    return eff, dict(frame=fr.words, aux=aux, tiles=tiles, rows=rows, flags=flags, n_cap=n_cap, listed=is_listed)


def _expected(sp: Spec, eff: dict, old: dict, oracle_mod) -> dict:
    """Every element of every output buffer after the call."""
    inp, P = sp.inp, sp.inp["P"]
    vis = (sp.radii > 0) & (sp.overflow == 0)
    keep = ~vis & (sp.prev_radii == 0 if sp.prev_radii is not None else False)
    zero = ~vis & ~keep & (not sp.accumulate)
    k = PR.chain_kwargs(inp)
    k.update(dL_dmean2D=eff["mean2D"], dL_dconic=eff["conic"], dL_dcolor=eff["color"], dL_ddepth=eff["depth"])
    if not sp.sh:
        k.update(shs=None)
    if sp.cov_precomp:
        k.update(scales=None, rotations=None, cov3D_precomp=sp.cov3D)
    o = oracle_mod.preprocess_backward(radii=vis.astype(np.int32), clamped=PR.clamp_bytes(sp.mask), cov3D=sp.cov3D, **k)
    new = dict(mean3D=o["means3D"], cov3D=o["cov3D"], scale=o["scales"], rot=o["rotations"])
    if sp.sh and sp.dsh:
        new["sh"] = o["sh"].reshape(P, -1)
    col = eff["color"]
    if sp.sh and not sp.dsh:  # factored mode: the clamp-masked colour gradient
        keepc = 1.0 - PR.clamp_bytes(sp.mask).astype(np.float32)
        col = (col * keepc).astype(np.float32)
    if sp.source != 0:
        m2 = eff["mean2D"].copy()
        m2[:, 2] = 0
        new.update(mean2D=m2, color=col, opacity=eff["opacity"].reshape(P, 1), semantic=eff["semantic"])
    elif sp.sh and not sp.dsh:
        new["color"] = col
    exp = {}
    for name, init in old.items():
        e = init.reshape(P, -1).copy()
        if name in new:
            n = new[name].reshape(P, -1)
            if sp.accumulate:
                s = (e + n).astype(np.float32)
                if name == "mean2D":
                    s[:, 2] = e[:, 2]
                e[vis] = s[vis]
            else:
                e[vis] = n[vis]
            if sp.source != 0 or name not in ("mean2D", "color"):  # (source 0: those two are the caller's inputs)
                e[zero] = 0.0
        exp[name] = e
    return exp


def run(sp: Spec, oracle_mod, *, check=True) -> dict:
    """Builds the buffers, calls the entry, compares every element of every output with the expectation.  Returns the outputs."""
    L = _L()
    lib = L.load()
    dev = "cuda"
    inp, P, S = sp.inp, sp.inp["P"], sp.S
    rng = np.random.default_rng(_seed(sp.tag))
    eff, src = _blend_gradients(sp, rng)
    M = inp["shs"].shape[1] if sp.sh else 0
    keepalive = []

    def D(a, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(dev)
        keepalive.append(t)
        return t

    i32 = lambda a: D(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))  # noqa: E731
    scene = L.GoiRasterScene()
    scene.P, scene.D, scene.M, scene.S, scene.W, scene.H = P, inp["sh_degree"], M, S, inp["W"], inp["H"]
    scene.means3D = D(inp["means3D"]).data_ptr()
    if sp.sh:
        scene.shs = D(inp["shs"]).data_ptr()
    else:
        scene.colors_precomp = D(np.zeros((P, 3), np.float32)).data_ptr()
    if sp.cov_precomp:
        scene.cov3D_precomp = D(sp.cov3D).data_ptr()
    else:
        scene.scales, scene.rotations = D(inp["scales"]).data_ptr(), D(inp["rotations"]).data_ptr()
    scene.scale_modifier = inp["scale_modifier"]
    scene.viewmatrix, scene.projmatrix = D(inp["viewmatrix"]).data_ptr(), D(inp["projmatrix"]).data_ptr()
    scene.campos = D(inp["campos"]).data_ptr()
    scene.tan_fovx, scene.tan_fovy = inp["tan_fovx"], inp["tan_fovy"]

    widths = dict(mean3D=3, cov3D=6, scale=3, rot=4, mean2D=3, color=3)
    if sp.sh and sp.dsh:
        widths["sh"] = 3 * M
    if sp.source == 0:
        widths.update(conic=4, depth=1)
    else:
        widths.update(opacity=1, semantic=S)
    orng = np.random.default_rng(_seed(sp.tag + "/old"))
    old = {n: (orng.normal(size=(P, w)).astype(np.float32) if sp.accumulate else np.full((P, w), NAN, np.float32))
           for n, w in widths.items()}
    if sp.source == 0:  # the per-id arrays are inputs
        up = inp["up"]
        old.update(mean2D=up["mean2D"].copy(), conic=up["conic"].copy(), color=up["color"].copy(), depth=up["depth"].reshape(P, 1).copy())
    out = {n: D(a) for n, a in old.items()}
    frame = i32(src["frame"]) if sp.source else i32(np.array([0, 0, sp.overflow], np.uint32))
    radii, clamped, cov3D = D(sp.radii, np.int32), D(sp.mask, np.uint8), D(sp.cov3D)
    prev = None if sp.prev_radii is None else D(sp.prev_radii, np.int32)
    aux = tiles = rows = flags = None
    n_cap = 0
    if sp.source:
        aux, tiles, rows, flags, n_cap = i32(src["aux"]), i32(src["tiles"]), D(src["rows"]), D(src["flags"]), src["n_cap"]
    ws = torch.full((256,), 0xA5, dtype=torch.uint8, device=dev)
    o = lambda n: _ptr(out.get(n))  # noqa: E731
    r = lib.goi_raster_debug_preprocess_backward(
        C.byref(scene), sp.source, 1 if sp.accumulate else 0, sp.max_blocks, n_cap, _ptr(frame), _ptr(radii), _ptr(clamped),
        None if sp.cov_precomp else _ptr(cov3D), _ptr(prev), _ptr(aux), _ptr(tiles), _ptr(rows), _ptr(flags), o("mean2D"), o("conic"),
        o("opacity"), o("color"), o("semantic"), o("depth"), o("mean3D"), o("cov3D"), o("sh"), o("scale"), o("rot"), _ptr(ws),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert r == 0, L.last_error()
    torch.cuda.synchronize()
    SEEN.add((bool(sp.sh and sp.dsh), sp.source))
    got = {n: t.cpu().numpy().reshape(P, -1) for n, t in out.items()}
    if rows is not None:  # the scratch is read, never written
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), src["rows"].view(np.uint32)), f"{sp.tag}: the row scratch changed"
    if check:
        exp = _expected(sp, eff, old, oracle_mod)
        vis = (sp.radii > 0) & (sp.overflow == 0)
        for name in got:
            bad = _bits(got[name]) != _bits(exp[name])
            if bad.any():
                g, j = (int(v) for v in np.argwhere(bad)[0])
                raise AssertionError(
                    f"{sp.tag}: dL_d{name}[{g}][{j}] = {got[name][g, j]!r} ({_bits(got[name])[g, j]:#010x}), expected "
                    f"{exp[name][g, j]!r} ({_bits(exp[name])[g, j]:#010x}); Gaussian {g} is "
                    f"{'visible' if vis[g] else 'invisible'}, clamp mask {int(sp.mask[g])}, {int(bad.any(1).sum())} rows differ "
                    f"({int(bad[vis].any(1).sum())} visible)")
    return got


# ---- inputs ---------------------------------------------------------------------------------------------------------------
_CACHE: dict = {}


def scene(oracle_mod, P, pose, **kw):
    """(inputs, the oracle forward's radii / clamp bits / cov3D) of a run, cached."""
    key = (P, pose, tuple(sorted(kw.items())))
    if key not in _CACHE:
        inp = PR.make_inputs(P, pose, **kw)
        radii, clamped, cov3D = PR.oracle_forward(oracle_mod, inp)
        _CACHE[key] = (inp, radii, PR.clamp_bits(clamped), cov3D)
    return _CACHE[key]


def spec(oracle_mod, P, pose, tag, *, visible=None, mask=None, scene_kw=None, **kw) -> Spec:
    """visible: None = what the oracle's forward sees, or a bool [P] / callable(P, rng) -> bool [P] (the outside pose only:
    every Gaussian lies in front of its camera)."""
    inp, radii, m, cov3D = scene(oracle_mod, P, pose, **(scene_kw or {}))
    if visible is not None:
        assert pose == "outside"
        depth = inp["means3D"].astype(np.float64) @ inp["viewmatrix"].reshape(4, 4)[:3, 2].astype(np.float64) + float(inp["viewmatrix"].reshape(4, 4)[3, 2])
        assert depth.min() > 1.0, "the outside pose keeps every Gaussian well in front of the near plane"
        v = visible(P, np.random.default_rng(_seed(tag + "/vis"))) if callable(visible) else np.asarray(visible)
        radii = np.where(v, np.maximum(radii, 1) + (np.arange(P) % 5), 0).astype(np.int32)
    if mask is not None:
        m = mask(P) if callable(mask) else np.asarray(mask, dtype=np.uint8)
    return Spec(inp, radii, m.astype(np.uint8), cov3D, tag, **kw)


# ---- arithmetic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ["inside", "corner", "narrow", "outside"])
@pytest.mark.parametrize("source", [0, 1, 2])
def test_scene_classes_bit_equal(oracle_mod, pose, source):
    """The camera inside the cloud, at a corner of the box, with a narrow field of view (frustum-clamped t.x / t.y, view depths
    down to 0.2, near-plane culls) and the canonical outside camera at an odd image size, from every source."""
    P = 3000 if pose == "outside" else 20000
    sp = spec(oracle_mod, P, pose, f"classes/{pose}/{source}", source=source, S=10 if source == 2 else 4)
    nvis = int((sp.radii > 0).sum())
    assert nvis >= 1000, nvis
    run(sp, oracle_mod)


@pytest.mark.parametrize("D,M", [(0, 16), (1, 16), (2, 16), (3, 16), (0, 1), (1, 4), (2, 9)])
@pytest.mark.parametrize("dsh", [True, False])
def test_sh_degrees_and_row_widths(oracle_mod, D, M, dsh):
    """M = 16: the 16-byte row fetch; M = 1, 4, 9: 3 M = 3, 12, 27 (the scalar fetch, and 12 the vector one again).  Coefficients
    above the active degree come out as exact zeros (the expectation holds +0 there)."""
    sp = spec(oracle_mod, 5000, "inside", f"sh/{D}/{M}/{dsh}", scene_kw=dict(sh_degree=D, M=M), dsh=dsh, max_blocks=2)
    got = run(sp, oracle_mod)
    if dsh and M > (D + 1) ** 2:
        vis = sp.radii > 0
        assert not _bits(got["sh"].reshape(sp.inp["P"], M, 3)[vis][:, (D + 1) ** 2:]).any()


@pytest.mark.parametrize("source", [0, 1, 2])
@pytest.mark.parametrize("dsh", [True, False])
def test_every_clamp_mask(oracle_mod, source, dsh):
    """Clamp masks 0 .. 7; without dL/dSH (factored mode) dL_dcolor must hold the masked gradient."""
    sp = spec(oracle_mod, 4000, "inside", f"clamp/{source}/{dsh}", mask=lambda P: (np.arange(P) * 7 % 8).astype(np.uint8),
              source=source, dsh=dsh, S=16 if source == 2 else 4)
    run(sp, oracle_mod)


@pytest.mark.parametrize("what", ["colors_precomp", "cov3D_precomp", "both", "modifier0.7", "modifier1.6", "qnorm"])
@pytest.mark.parametrize("source", [0, 1])
def test_optional_paths(oracle_mod, what, source):
    """colors_precomp: no SH path (dL_dcolor passed through / written from the record); cov3D_precomp: no scale / rotation path
    (dL_dcov3D is the result, dL_dscale and dL_drot zeros); scale_modifier 0.7 and 1.6; quaternions of norm 0.5 .. 2."""
    kw, skw = {}, {}
    if what in ("colors_precomp", "both"):
        kw.update(sh=False, dsh=False)
    if what in ("cov3D_precomp", "both"):
        kw.update(cov_precomp=True)
    if what.startswith("modifier"):
        skw.update(scale_modifier=float(what[8:]))
    if what == "qnorm":
        skw.update(qnorm=True)
    run(spec(oracle_mod, 6000, "inside", f"optional/{what}/{source}", scene_kw=skw, source=source, **kw), oracle_mod)


# ---- control flow -----------------------------------------------------------------------------------------------------------
def _all(P, rng):
    return np.ones(P, dtype=bool)


SIZES = [1, 208, 209, 223, 224, 225, 255, 256, 257, 479, 480, 1000, 5000]


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("source", [0, 1, 2])
def test_sizes_around_the_tile_and_segment_boundaries(oracle_mod, P, source):
    """Everything visible (tiles of 224 / 208 rows fill up and split) and, in a second call, a random half."""
    for frac in (1.0, 0.5):
        sp = spec(oracle_mod, P, "outside", f"sizes/{P}/{source}/{frac}", visible=lambda n, rng: rng.random(n) < frac,
                  source=source, S=16 if source == 2 else 3, max_blocks=1 if P == 5000 else 0)
        run(sp, oracle_mod)


def test_the_products_grid_makes_second_trips(oracle_mod):
    """P above 3 x 256 x CUs: the product's own grid (max_blocks 0) walks more than one segment per workgroup."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P = 3 * 256 * cus + 256 * 37 + 19
    sp = spec(oracle_mod, P, "outside", "large", visible=lambda n, rng: rng.random(n) < 0.51, source=1, S=16)
    run(sp, oracle_mod)


PATTERNS = {
    "all": _all,
    "none": lambda P, rng: np.zeros(P, dtype=bool),
    "every2nd": lambda P, rng: np.arange(P) % 2 == 0,
    "every7th": lambda P, rng: np.arange(P) % 7 == 3,
    "one_per_segment": lambda P, rng: np.arange(P) % 256 == 131,
    # a dense run whose last id fills a tile exactly: 2 x 224 (2 x 208 on the fused path is covered by "run416")
    "run448": lambda P, rng: (np.arange(P) >= 100) & (np.arange(P) < 100 + 448),
    "run416": lambda P, rng: (np.arange(P) >= 300) & (np.arange(P) < 300 + 416),
    "last": lambda P, rng: np.arange(P) == P - 1,
    "last3": lambda P, rng: np.arange(P) >= P - 3,
    "frac8": lambda P, rng: rng.random(P) < 0.08,
    "frac51": lambda P, rng: rng.random(P) < 0.51,
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("max_blocks", [1, 2, 3])
def test_visibility_patterns_with_few_workgroups(oracle_mod, pattern, max_blocks):
    """5000 Gaussians walked by 1, 2 or 3 workgroups (20, 10 or 7 segments each: the pending list carries over), from the
    source the product uses (1) and, for one grid, the other two; the result must not depend on the grid."""
    outs = []
    for source in ((0, 1, 2) if max_blocks == 1 else (1,)):
        sp = spec(oracle_mod, 5000, "outside", f"pattern/{pattern}/{source}", visible=PATTERNS[pattern], source=source,
                  S=10 if source == 2 else 16, max_blocks=max_blocks)
        outs.append((source, sp, run(sp, oracle_mod)))
    if max_blocks == 1:  # the same call on the product's grid and once more: bit-identical
        source, sp, a = outs[1]
        for mb in (0, 1):
            sp.max_blocks = mb
            b = run(sp, oracle_mod, check=False)
            for n in a:
                assert np.array_equal(_bits(a[n]), _bits(b[n])), f"{pattern}: dL_d{n} differs with max_blocks {mb}"


@pytest.mark.parametrize("source,dsh", [(0, True), (0, False), (1, True), (1, False), (2, True), (2, False)])
@pytest.mark.parametrize("prev", [None, "mixed"])
def test_invisible_rows_zero_or_untouched(oracle_mod, source, dsh, prev):
    """Without prev_radii an invisible Gaussian gets zeros in every output of the instantiation (dL_dsh and dL_dsemantic
    included); with it, the NaN it held stays where prev_radii == 0 and zeros come where prev_radii > 0.  (run() compares every
    element of every buffer with exactly that expectation.)"""
    P = 3000
    pr = None if prev is None else np.where(np.arange(P) % 3 == 0, 0, 7).astype(np.int32)
    sp = spec(oracle_mod, P, "outside", f"invisible/{source}/{dsh}/{prev}", visible=PATTERNS["frac51"], source=source, dsh=dsh,
              S=20 if source == 2 else 17, prev_radii=pr, max_blocks=2)
    got = run(sp, oracle_mod)
    inv = sp.radii == 0
    names = ["mean3D", "cov3D", "scale", "rot"] + (["sh"] if dsh else []) + (["opacity", "semantic", "mean2D", "color"] if source else [])
    for n in names:
        if pr is None:
            assert not _bits(got[n][inv]).any(), n
        else:
            assert np.isnan(got[n][inv & (pr == 0)]).all() and not _bits(got[n][inv & (pr > 0)]).any(), n


@pytest.mark.parametrize("source,dsh", [(0, True), (1, True), (1, False), (2, True)])
@pytest.mark.parametrize("prev", [None, "mixed"])
def test_truncated_frame_back_propagates_nothing(oracle_mod, source, dsh, prev):
    """A non-zero overflow word: every row zero (or kept, by the prev_radii rule), whatever radii says."""
    P = 2000
    pr = None if prev is None else np.where(np.arange(P) % 4 == 1, 0, 3).astype(np.int32)
    sp = spec(oracle_mod, P, "outside", f"overflow/{source}/{dsh}/{prev}", visible=_all, source=source, dsh=dsh,
              S=10 if source == 2 else 4, overflow=1 + (source == 1), prev_radii=pr)
    got = run(sp, oracle_mod)
    for n in ("mean3D", "cov3D", "scale", "rot"):
        assert not np.nan_to_num(got[n], nan=0.0).any(), n
        assert np.isnan(got[n]).any(1).sum() == (0 if pr is None else int((pr == 0).sum())), n


@pytest.mark.parametrize("S", [4, 10, 17])
@pytest.mark.parametrize("max_blocks", [0, 1])
def test_accumulate_adds_to_visible_rows_only(oracle_mod, S, max_blocks):
    """Outputs pre-filled with a known array: visible rows = old + new (that fp32 sum, bit for bit), invisible rows unchanged."""
    sp = spec(oracle_mod, 5000, "outside", f"accumulate/{S}/{max_blocks}", visible=PATTERNS["frac51"], source=1, S=S,
              accumulate=True, max_blocks=max_blocks)
    run(sp, oracle_mod)


@pytest.mark.parametrize("S", list(range(1, 33)))
def test_records_listed_and_unlisted(oracle_mod, S):
    """Source 1: visible Gaussians with a record and without (tiles_touched == 0: zero blend gradients, the chain still runs);
    dL_dsemantic leaves as float4 (S % 4 == 0) or scalar copies, from records of 16, 32 and 48 floats: every width admitted."""
    sp = spec(oracle_mod, 3000, "outside", f"records/{S}", visible=PATTERNS["frac51"], source=1, S=S, listed=0.6, max_blocks=3)
    got = run(sp, oracle_mod)
    vis, listed = sp.radii > 0, sp.extra["listed"]
    assert (vis & listed).sum() > 500 and (vis & ~listed).sum() > 300
    assert not _bits(got["semantic"][vis & ~listed]).any() and not _bits(got["opacity"][vis & ~listed]).any()
    for n in ("mean3D", "cov3D", "scale", "rot", "sh"):  # zero blend gradients in, zeros (of either sign) out: written, not NaN
        assert not got[n][vis & ~listed].any(), n
    assert np.abs(got["sh"][vis & listed]).max() > 0


@pytest.mark.parametrize("S", list(range(5, 21)))
@pytest.mark.parametrize("dense", [False, True])
def test_rows_summed_in_the_kernel(oracle_mod, S, dense):
    """Source 2: unflagged rows, rows past the count and the padding hold NaN; Gaussians on both sides of the frame's
    big-instance threshold (a big one's record is read instead of its rows), on a sparse and on a dense frame; every width the
    source admits (128-byte rows: S = 5 .. 20; the float2 store of an even S and the scalar one of an odd S)."""
    sparse, big = K["SPARSE_INST"], K["BIG_INST"]
    counts = (big, big + 1, big + 40) if dense else (sparse, sparse + 1, big + 1, 700)
    sp = spec(oracle_mod, 2500, "outside", f"rows/{S}/{dense}", visible=PATTERNS["frac51"], source=2, S=S, listed=0.7,
              big=counts, dense=dense, max_blocks=2)
    run(sp, oracle_mod)
    assert sp.extra["big_inst"] == (big if dense else sparse), sp.extra
    assert sp.extra["n_big"] == (2 if dense else 1)


def test_refusals():
    """Invalid combinations are refused by name, before anything is launched."""
    L = _L()
    lib = L.load()
    P = 16
    z = torch.zeros(P * 48, dtype=torch.float32, device="cuda")
    zi = torch.zeros(P * 4, dtype=torch.int32, device="cuda")
    ws = torch.zeros(512, dtype=torch.uint8, device="cuda")

    def call(*, source=0, flags=0, max_blocks=0, n_cap=8, S=4, prev=None, dsh=True, M=16, D=3, ws_off=0, cov_precomp=False,
             scales=True, conic=True):
        sc = L.GoiRasterScene()
        sc.P, sc.D, sc.M, sc.S, sc.W, sc.H = P, D, M, S, 64, 48
        sc.means3D = sc.shs = sc.viewmatrix = sc.projmatrix = sc.campos = z.data_ptr()
        if scales:
            sc.scales = sc.rotations = z.data_ptr()
        if cov_precomp:
            sc.cov3D_precomp = z.data_ptr()
        sc.tan_fovx = sc.tan_fovy = 0.5
        p, pi = _ptr(z), _ptr(zi)
        return lib.goi_raster_debug_preprocess_backward(
            C.byref(sc), source, flags, max_blocks, n_cap, pi, pi, pi, p, _ptr(prev), pi, pi, p, pi, p, p if conic else None, p, p, p,
            p, p, p, p if dsh else None, p, p, C.c_void_p(ws.data_ptr() + ws_off), None)

    def refused(needle, **kw):
        assert call(**kw) < 0, kw
        msg = L.last_error()
        assert msg.startswith("goi_raster_debug_preprocess_backward:") and needle in msg, msg

    refused("unknown source", source=3)
    refused("unknown flag", flags=2)
    refused("max_blocks", max_blocks=-1)
    refused("128-byte rows", source=2, S=4)
    refused("128-byte rows", source=2, S=21)
    refused("accumulate needs source 1", flags=1, source=0)
    refused("accumulate needs source 1", flags=1, source=2, S=10)
    refused("accumulate with prev_radii", flags=1, source=1, prev=zi)
    refused("accumulate with factored SH", flags=1, source=1, dsh=False)
    refused("SH degree", M=4, D=3)
    refused("SH degree", M=17)
    refused("256-byte aligned", ws_off=64)
    refused("exactly one of", cov_precomp=True)
    refused("exactly one of", scales=False)
    refused("source 0 reads", conic=False)
    refused("need 1 <= S <= 32", S=33)
    assert call() == 0 and call(source=1) == 0 and call(source=2, S=10) == 0  # (all-zero radii: nothing is visible)
    torch.cuda.synchronize()


def test_every_instantiation_was_launched():
    """(runs last in the module) all six instantiations of preprocess_bwd_k appeared above."""
    want = {(d, s) for d in (True, False) for s in (0, 1, 2)}
    if SEEN:  # (a run of this test alone has seen nothing)
        assert want <= SEEN, sorted(want - SEEN)
