"""The blend kernels called directly -- pair evaluation, member masks, row slots, validity bytes and every element of every
backward row -- against the float64 reference of tests/blend_reference.py.

Two test hooks of the C ABI (include/goi_raster.h) run the product's own launchers and device functions:
  * goi_raster_debug_pair_eval: E, alpha and the two guard bits of the 64 pixels of caller-chosen (Gaussian, quadrant) pairs through
    poly_coefs / eval_poly (csrc/blend_common.h), the one function pair every blend kernel evaluates a pair with;
  * goi_raster_debug_backward_blend: the backward blend stage alone on a real frame, in every form of the kernel, with the row
    scratch, the validity bytes, the aux words, the member masks, qcost and qorder copied out.
goi_raster_debug_views supplies records, lists, ranges and n_contrib.  The reference takes the kernel's own alphas and last
contributors as inputs, so NO row and NO pixel is excluded anywhere.

PAIR EVALUATION (default build; skipped under GOI_ALPHA_DIRECT, whose form this bound does not describe).  alpha == min(0.99f, E)
and seen == (alpha >= fp32(1/255)) exactly; `below` agrees with float64 outside the band of the exponent's error bound;
|log2 E - P64| <= 18 x 2^-24 x (sum of the magnitudes of the polynomial's terms) + the v_exp_f32 ulp, the 18 roundings counted at
blend_reference.PAIR_ROUNDINGS; for the sharpest admissible conic (a = c = 1/0.3) the error stays under the 5e-5 the kernel header
claims.  Cases: tests/blend_cases.py::pair_cases (both sides of the S = 16 switch to fp64 coefficients, needles up to 800 pixels long,
opacity 0 and around 1/255, centres on pixels, lanes outside the image) and every candidate pair of every frame below.

FORWARD, given the dumped pair bits: qcost == the quadrant's largest n_contrib; member bit == "some pixel has the position below its
n_contrib and passes both guards" for every position below qcost; n_contrib consistent with the stop rule in float64 within
(k + 2) 2^-23; out_alpha and the four maps within the magnitude companion times the gate.

BACKWARD ROWS.  Validity byte 1 exactly on the slots of member pairs -- slot = (first[g] + rank of the tile among g's listed tiles) x 4
+ quadrant, the rank read off point_list / ranges, first[g] from aux and checked to partition [0, N) -- and 0 on every other slot;
padded semantic channels exactly 0; every element within blend_reference.element_tolerance: the derived operand-split term plus the
MEASURED gate -- 4 x median and 99th percentile, 16 x maximum of the float32 yardstick's normalised error per element class, pooled
over the cases (blend_reference.GATE, measured on the CPU with tools/blend_yardstick.py: docs/MEASUREMENT_LOG.md, "Direct test of
the blend kernels") -- under the hard ceiling (n_terms + 3 depth) 2^-24 M.  The kernel's own output never sets a tolerance.
Default mode (split-f16 flush, member masks) on every run of blend_cases.all_runs(); the exact-fp32 flush, candidate testing, the
semantic-only rows and the per-tile kernel's per-id arrays on a subset.

CHAIN LINK.  At bwd_records 0 the per-id outputs of the ordinary backward equal, bit for bit, the dumped rows added up in the order of
tests/reduce_rows_reference.py: the three direct tests (blend rows, row reduction, per-Gaussian backward) meet.

EVERY SEMANTIC WIDTH.  The frame of tests/channel_count_cases.py at each S = 1..32 (every S4 instantiation, the 16-byte and the
scalar row path, 1 and 2 accumulator blocks, rows of 16 / 32 / 48 floats): pair evaluation, forward and default rows at every width;
the other forms of the row kernel, the semantic-only rows in all four forms and the per-tile kernel at 4 S4 - 1 and 4 S4; the chain
link and the record paths (bwd_records 1, 2 against 0) at every width.  Same reference, same tolerances.

Nothing here is built to make a kernel fault: every frame is a valid forward of the product.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import blend_cases as BC
from tests import blend_reference as BR
from tests import channel_count_cases as CC
from tests import raw_frame
from tests import reduce_rows_reference as RR
from tests.raw_frame import ptr as _ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA_DIRECT = "GOI_ALPHA_DIRECT" in os.environ.get("GOI_EXTRA_FLAGS", "")
DEV = "cuda"
STATS = {}


def _artefact_dir():
    with open(os.path.join(ROOT, ".gitignore")) as fh:
        names = [line.strip().rstrip("/") for line in fh if line.strip().endswith("_out/")]
    assert len(names) == 1, names
    return os.path.join(ROOT, names[0])


@pytest.fixture(scope="module", autouse=True)
def _stats_file():
    t0 = time.time()
    yield
    out = _artefact_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "blend_rows_stats.json"), "w") as fh:
        json.dump(dict(stats=STATS, module_wall_seconds=round(time.time() - t0, 1)), fh, indent=1, sort_keys=True, default=float)


def _L():
    from goi_hyperplane_amd import _lib
    return _lib


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


# ---- a frame on the device -------------------------------------------------------------------------------------------------
class DeviceFrame(raw_frame.RawFrame):
    """One exact forward of the product through the C ABI, its workspaces kept, and what the reference needs of it."""

    def __init__(self, sc, cam, bg):
        super().__init__(sc, cam, bg, DEV)
        lib, P, S, W, H = self.lib, self.P, self.S, self.W, self.H
        self.frame = self.quads = None
        if self.N == 0:
            return
        v = {k: x.cpu().numpy() for k, x in self.views().items()}
        self.frame = BR.Frame(W, H, S, v["means2D"], v["conic_opacity"], v["rgb"], v["depths"], np.asarray(sc.semantics, np.float32),
                              v["point_list"].astype(np.uint32), v["ranges"].astype(np.uint32), v["n_contrib"].astype(np.uint32),
                              self.alpha.cpu().numpy().reshape(-1), np.asarray(bg, np.float32))
        self.quads = BR.candidates(self.frame)
        self.E, self.al, self.guards = pair_eval(lib, P, W, H, self.geom, BR.requests(self.quads))
        self.hit = (self.guards & 3) == 3

    def maps(self):
        return dict(color=self.color.cpu().numpy(), sem=self.semmap.cpu().numpy(), depth=self.depth.cpu().numpy(),
                    alpha=self.alpha.cpu().numpy())

    def blend(self, mode: int, up: dict, nan_fill=True):
        """goi_raster_debug_backward_blend -> dict of host arrays."""
        lib, P, S, W, H, N = self.lib, self.P, self.S, self.W, self.H, self.N
        T4 = self.quads.Q
        tile, sem = mode == 8, (mode & 4) != 0 and mode != 8
        rf = lib.goi_raster_debug_reduce_row_floats(3 if sem else 1, S)
        scratch = torch.full((lib.goi_raster_backward_scratch_bytes(N, S),), 0xFF, dtype=torch.uint8, device=DEV)  # (NaN rows)
        o = dict(rows=torch.zeros((4 * N, rf), device=DEV), flags=torch.full((4 * N,), 7, dtype=torch.uint8, device=DEV),
                 aux=torch.zeros((P, 4), dtype=torch.int32, device=DEV), qmask0=torch.zeros(T4, dtype=torch.int64, device=DEV),
                 qmask=torch.zeros(4 * (N // 64 + 2), dtype=torch.int64, device=DEV),
                 qcost=torch.zeros(T4, dtype=torch.int32, device=DEV), qorder=torch.full((8 * ((T4 + 7) // 8),), -2, dtype=torch.int32, device=DEV))
        arr = dict(mean2D=(P, 3), conic=(P, 4), opacity=(P,), color=(P, 3), semantic=(P, S), depth=(P,))
        a = {k: torch.full(s, float("nan"), device=DEV) for k, s in arr.items()} if tile else {k: None for k in arr}
        ups = [_dev(up.get(k)) for k in ("color", "sem", "depth", "alpha")]
        r = lib.goi_raster_debug_backward_blend(
            C.byref(self.scene), N, mode, _ptr(self.geom), _ptr(self.binning), _ptr(self.img), _ptr(self.radii), _ptr(self.alpha),
            *[_ptr(u) for u in ups], None if tile else _ptr(scratch), None if tile else _ptr(o["rows"]),
            None if tile else _ptr(o["flags"]), _ptr(o["aux"]), _ptr(o["qmask0"]), _ptr(o["qmask"]), _ptr(o["qcost"]), _ptr(o["qorder"]),
            *[_ptr(a[k]) for k in ("mean2D", "conic", "opacity", "color", "semantic", "depth")], None)
        assert r >= 0, _L().last_error()
        torch.cuda.synchronize()
        out = {k: x.cpu().numpy() for k, x in o.items()}
        out["qmask0"], out["qmask"] = out["qmask0"].view(np.uint64), out["qmask"].view(np.uint64)
        out["aux"] = out["aux"].view(np.uint32)
        out["ordered"] = r
        out.update({k: x.cpu().numpy() for k, x in a.items() if x is not None})
        return out


def pair_eval(lib, P, W, H, geom, req):
    n = len(req)
    rq = _dev(req.astype(np.uint32).view(np.int32))
    E, al = torch.full((n, 64), -1.0, device=DEV), torch.full((n, 64), -1.0, device=DEV)
    gd = torch.full((n, 64), 0x40, dtype=torch.uint8, device=DEV)
    assert lib.goi_raster_debug_pair_eval(P, W, H, _ptr(geom), _ptr(rq), n, _ptr(E), _ptr(al), _ptr(gd), None) >= 0, _L().last_error()
    torch.cuda.synchronize()
    gd = gd.cpu().numpy()
    assert not (gd & 0x40).any(), "a requested pair was not written"
    return E.cpu().numpy(), al.cpu().numpy(), gd


def _check_pairs_chunked(fr, qd, E, al, gd, chunk=40000):
    worst = dict(n=0, max_err=0.0, max_ratio=0.0, n_wide=0, max_err_wide=0.0, max_terms=0.0)
    for lo in range(0, qd.npairs, chunk):
        sel = np.arange(lo, min(lo + chunk, qd.npairs))
        r = BR.check_pairs(fr, qd, E[sel], al[sel], gd[sel], sel, check_bound=not ALPHA_DIRECT)
        for k, v in r.items():
            worst[k] = worst[k] + v if k in ("n", "n_wide") else max(worst[k], v)
    return worst


# ---- pair evaluation on written records ----------------------------------------------------------------------------------------
@pytest.mark.skipif(ALPHA_DIRECT, reason="the bound describes the default build's folded polynomial")
def test_pair_evaluation_against_float64_on_constructed_records():
    lib = _L().load()
    m, co, W, H = BC.pair_cases()
    P = len(m)
    # the records are the first array of the geometry workspace: [P] x (x, y, a, b | c, opacity, hx, hy | r, g, b, depth)
    geom = torch.zeros(lib.goi_raster_geom_bytes(P), dtype=torch.uint8, device=DEV)
    rec = np.zeros((P, 12), np.float32)
    rec[:, 0:2], rec[:, 2:4], rec[:, 4:6] = m, co[:, 0:2], co[:, 2:4]
    geom[:P * 48] = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(DEV)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    Q = 4 * gx * gy
    fr = BR.Frame(W, H, 1, m, co, np.zeros((P, 3), np.float32), np.zeros(P, np.float32), np.zeros((P, 1), np.float32),
                  np.tile(np.arange(P, dtype=np.uint32), gx * gy), np.stack([np.arange(gx * gy) * P, np.arange(1, gx * gy + 1) * P], 1),
                  np.zeros(W * H, np.uint32), np.zeros(W * H, np.float32), BC.BG0)
    qd = BR.candidates(fr)  # every Gaussian against every quadrant
    assert qd.npairs == P * Q
    E, al, gd = pair_eval(lib, P, W, H, geom, BR.requests(qd))
    r = BR.check_pairs(fr, qd, E, al, gd)
    p = BR.poly64(fr, qd)
    assert (p["S"] < 16).any() and (p["S"] >= 16).any() and r["n_wide"] > 0
    assert (~qd.inside[qd.pair_quad]).any(), "no lane outside the image"
    sharp = (co[qd.pair_id, 0] > 3.3) & (co[qd.pair_id, 2] > 3.3)
    ok = sharp[:, None] & (E > 2.0 ** -120)
    err = np.abs(np.log2(E.astype(np.float64), where=ok, out=np.zeros(E.shape)) - p["P"])[ok]
    STATS["pairs/constructed"] = dict(r, sharp_max_err=float(err.max()), sharp_n=int(ok.sum()))
    print("pairs/constructed", STATS["pairs/constructed"])
    assert err.max() <= 5e-5, f"the sharpest conic's exponent is {err.max():.3e} off (the kernel header claims <= 5e-5)"
    # a request that names no Gaussian / no quadrant writes NaN and 0x80, and nothing else
    bad = np.array([[P, 0], [0, Q], [0xFFFFFFFF, 0xFFFFFFFF], [1, 1]], np.uint32)
    E2, al2, gd2 = pair_eval(lib, P, W, H, geom, bad)
    assert np.isnan(E2[:3]).all() and np.isnan(al2[:3]).all() and (gd2[:3] == 0x80).all() and not (gd2[3] & 0x80).any()


# ---- frames ------------------------------------------------------------------------------------------------------------------
_FRAMES = {}


def _frame(name, bg):
    key = (name, tuple(np.asarray(bg).tolist()))
    if key not in _FRAMES:
        _FRAMES.clear()  # (one frame at a time: the 400 x 300 case holds a few hundred MB of dumped pairs)
        sc, cam = BC.ROW_CASES[name]()
        _FRAMES[key] = DeviceFrame(sc, cam, bg)
    return _FRAMES[key]


def _rows_of(out, slots, ncol):
    return np.asarray(out["rows"])[slots][:, :ncol]


def test_forward_and_default_backward_rows_on_every_case():
    """Every run of blend_cases.all_runs(): pair evaluation of every candidate pair, the forward's qcost / member masks / n_contrib /
    maps, and the default backward's slots, validity bytes and row elements; then the pooled gate."""
    S_list, errs, raw_errs, y_errs, failures = [], [], [], [], []
    covered = dict(carry=False, rounds=False, wide=False, outside_quadrant=False, saturated=False)
    for name, kind in BC.all_runs():
        tag = f"{name}/{kind}"
        try:
            sc, cam = BC.ROW_CASES[name]()
            up, bg = BC.upstream(kind, sc.S, cam.image_height, cam.image_width, name)
            df = _frame(name, bg)
            assert df.N > 0, "the case renders nothing"
            fr, qd = df.frame, df.quads
            st = dict(N=df.N, pairs=qd.npairs)
            if kind == "random" or kind == "bg":
                st["pair_eval"] = _check_pairs_chunked(fr, qd, df.E, df.al, df.guards)
                covered["wide"] |= st["pair_eval"]["n_wide"] > 0
            out = df.blend(0, up)
            if kind == "random" or kind == "bg":
                BR.check_masks(qd, df.hit, out["qmask0"], out["qmask"], out["qcost"])
                st["forward"] = BR.check_forward(fr, qd, BR.forward_reference(fr, qd, df.al, df.hit), df.maps(), BR.GATE)
            ref = BR.backward_rows(fr, qd, up, df.E, df.al, df.hit)
            slots = BR.slots_reference(fr, qd, out["aux"])
            BR.check_flags(slots, ref.member, out["flags"], df.N)
            ncol = BR.nsem_of(sc.S) + 10
            got = np.zeros((qd.npairs, ncol), np.float32)
            got[ref.member] = _rows_of(out, slots[ref.member], ncol)
            err = BR.check_rows(sc.S, qd, ref, got, BR.GATE, tag)
            S_list.append(sc.S)
            errs.append(err)
            raw_errs.append(BR.normalised_errors(sc.S, ref, got)[0])  # (the derived feature term not taken off: for the log)
            st["rows"] = int(ref.member.sum())
            st["depth"] = int(ref.depth.max())
            st["kernel"] = {c: [x / BR.U for x in v[:3]] for c, v in BR.class_stats(sc.S, err).items()}
            if name != "masks-400x300":  # (the yardstick on the device's alphas, for the log; the largest case is left out for time)
                y = BR.backward_rows(fr, qd, up, df.E, df.al, df.hit, dtype=np.float32)
                ey, _ = BR.normalised_errors(sc.S, ref, y.rows)
                y_errs.append((sc.S, ey))
                st["yardstick"] = {c: [x / BR.U for x in v[:3]] for c, v in BR.class_stats(sc.S, ey).items()}
            members_per_quad = np.bincount(qd.pair_quad[ref.member], minlength=qd.Q)
            covered["carry"] |= bool(((members_per_quad > 32) & (members_per_quad % 8 != 0)).any())
            covered["rounds"] |= bool((qd.qmax > 64).any())
            covered["outside_quadrant"] |= bool((~qd.inside).all(axis=1).any())
            covered["saturated"] |= bool((qd.nc.max(axis=1) < qd.length).any())
            STATS[tag] = st
            print(tag, json.dumps(st, default=float), flush=True)
        except AssertionError as ex:
            failures.append(f"{tag}: {ex}")
            print("FAILED", tag, ex, flush=True)
    pooled = BR.pooled_stats(S_list, errs)
    STATS["pooled/kernel"] = {c: [x / BR.U for x in v[:3]] + [v[3]] for c, v in pooled.items()}
    STATS["pooled/kernel_raw"] = {c: [x / BR.U for x in v[:3]] + [v[3]] for c, v in BR.pooled_stats(S_list, raw_errs).items()}
    if y_errs:
        py = BR.pooled_stats([s for s, _ in y_errs], [e for _, e in y_errs])
        STATS["pooled/yardstick_device_alphas"] = {c: [x / BR.U for x in v[:3]] + [v[3]] for c, v in py.items()}
        STATS["pooled/ratio_kernel_to_yardstick"] = {c: [pooled[c][i] / py[c][i] if py[c][i] else 0.0 for i in range(3)] for c in BR.CLASSES}
    print("pooled", json.dumps({k: v for k, v in STATS.items() if k.startswith("pooled/")}, default=float), flush=True)
    assert not failures, "\n".join(failures)
    assert all(covered.values()), covered
    BR.check_gate(pooled, BR.GATE, "default mode: ")


SUBSET = ("S3", "S16", "S17", "ragged-123x77", "huge-64x48", "stack-33", "stack-129", "opaque-65")


def _subset_cases(names=SUBSET):
    """(tag, scene, frame, upstream gradients) of the named row cases under random gradients"""
    for name in names:
        sc, cam = BC.ROW_CASES[name]()
        up, bg = BC.upstream("random", sc.S, cam.image_height, cam.image_width, name)
        yield name, sc, _frame(name, bg), up


def _other_form(mode, what, cases, key):
    pooled_S, pooled_e = [], []
    for name, sc, df, up in cases:
        fr, qd = df.frame, df.quads
        out = df.blend(mode, up)
        ref = BR.backward_rows(fr, qd, up, df.E, df.al, df.hit)
        slots = BR.slots_reference(fr, qd, out["aux"])
        BR.check_flags(slots, ref.member, out["flags"], df.N)
        ncol = BR.nsem_of(sc.S) + 10
        got = np.zeros((qd.npairs, ncol), np.float32)
        got[ref.member] = _rows_of(out, slots[ref.member], ncol)
        pooled_e.append(BR.check_rows(sc.S, qd, ref, got, BR.GATE, f"{name}/mode {mode}", split=(mode & 1) == 0))
        pooled_S.append(sc.S)
        if mode == 2:  # the member-mask walk and the candidate-testing walk flush the same pairs in the same order: same bits
            d = df.blend(0, up)
            a, b = _rows_of(d, slots[ref.member], ncol), _rows_of(out, slots[ref.member], ncol)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: bwd_masks 0 and 1 differ"
    pooled = BR.pooled_stats(pooled_S, pooled_e)
    STATS[key] = {c: [x / BR.U for x in v[:3]] + [v[3]] for c, v in pooled.items()}
    print(what, STATS[key])
    BR.check_gate(pooled, BR.GATE, f"{what}: ")


OTHER_FORMS = [(1, "exact-fp32 flush"), (2, "candidate testing"), (3, "exact-fp32 flush, candidate testing")]


@pytest.mark.parametrize("mode,what", OTHER_FORMS)
def test_other_forms_of_the_row_kernel(mode, what):
    _other_form(mode, what, _subset_cases(), f"pooled/mode{mode}")


def _semantic_only_rows(cases, modes):
    for name, sc, df, up in cases:
        fr, qd = df.frame, df.quads
        n = BR.nsem_of(sc.S)
        ref = BR.backward_rows(fr, qd, dict(sem=up["sem"]), df.E, df.al, df.hit)
        for mode in modes:
            out = df.blend(mode, dict(sem=up["sem"]))
            slots = BR.slots_reference(fr, qd, out["aux"])
            BR.check_flags(slots, ref.member, out["flags"], df.N)
            got = np.zeros((qd.npairs, n + 10), np.float32)
            got[ref.member, :n] = _rows_of(out, slots[ref.member], n)
            got[ref.member, n:] = ref.rows[ref.member, n:]  # (not produced by this kernel)
            BR.check_rows(sc.S, qd, ref, got, BR.GATE, f"{name}/mode {mode}", split=(mode & 1) == 0)


def test_semantic_only_rows():
    """render_bwd_sem_k: rows of the padded semantic channels alone, same slots, same validity bytes, the feature tolerance."""
    _semantic_only_rows(_subset_cases(), (4, 5))


def _per_tile_arrays(cases):
    for name, sc, df, up in cases:
        fr, qd = df.frame, df.quads
        out = df.blend(8, up)
        ref = BR.backward_rows(fr, qd, up, df.E, df.al, df.hit)
        n = BR.nsem_of(sc.S)
        tol_rows = BR.element_tolerance(sc.S, qd, ref, BR.GATE, split=False)
        tol_rows[:, n + 4:] *= 4.6
        want, tol = BR.per_gaussian_sums(fr, qd, ref), np.zeros((fr.P, n + 10))
        np.add.at(tol, qd.pair_id[ref.member], tol_rows[ref.member])
        nrows = np.bincount(qd.pair_id[ref.member], minlength=fr.P)
        mag = np.zeros((fr.P, n + 10))
        np.add.at(mag, qd.pair_id[ref.member], ref.mag[ref.member])
        tol += (nrows[:, None] + 4) * BR.U * mag  # (the atomic additions themselves)
        emap, _ = RR.element_map(sc.S, 0, BR.row_floats(sc.S))
        arrays = {k: out[k].reshape(fr.P, -1) for k in ("mean2D", "conic", "opacity", "color", "semantic", "depth")}
        assert arrays["semantic"].shape == (fr.P, sc.S)
        for el in range(n + 10):
            if emap[el] is None:
                continue
            a, col = emap[el]
            d = np.abs(arrays[a][:, col].astype(np.float64) - want[:, el])
            assert np.isfinite(arrays[a]).all(), (name, a)
            assert (d <= tol[:, el]).all(), (name, a, col, float((d - tol[:, el]).max()), int(np.argmax(d - tol[:, el])))
        assert not arrays["mean2D"][:, 2].any() and not arrays["conic"][:, 2].any()


def test_per_tile_kernel_arrays():
    """render_bwd_tile_k: the six per-id arrays against the per-Gaussian float64 sums of the reference's rows.  The kernel adds the
    quadrants' partial sums with atomics (any order) and expands its moments around the TILE centre (|u|, |v| <= 7.5): an element
    may be off by the sum of its rows' tolerances, the moment-derived ones by 4.6 times that ((7.5 / 3.5)^2 < 4.6: the squares of the
    basis; the companions here carry the quadrant-centred basis)."""
    _per_tile_arrays(_subset_cases(("S3", "S16", "ragged-123x77", "stack-33")))


_GRAD_NAMES = ("mean2D", "conic", "opacity", "color", "semantic", "depth", "mean3D", "cov3D", "sh", "scale", "rot")


def _raw_backward(df, sc, up, records):
    """goi_raster_backward of the frame at bwd_records `records`, every output NaN before the call -> dict of host arrays"""
    L = _L()
    lib = L.load()
    P, S, N = df.P, df.S, df.N
    M = sc.shs.shape[1]
    shapes = dict(mean2D=(P, 3), conic=(P, 4), opacity=(P,), color=(P, 3), semantic=(P, S), depth=(P,), mean3D=(P, 3), cov3D=(P, 6),
                  sh=(P, M, 3), scale=(P, 3), rot=(P, 4))
    g = {k: torch.full(s, float("nan"), device=DEV) for k, s in shapes.items()}
    scratch = torch.empty(lib.goi_raster_backward_scratch_bytes(N, S), dtype=torch.uint8, device=DEV)
    ups = [_dev(up[k]) for k in ("color", "sem", "depth", "alpha")]
    before = dict(L.OPTIONS)
    try:
        L.set_option("bwd_records", records)
        r = lib.goi_raster_backward(C.byref(df.scene), N, 0, 0, _ptr(df.geom), _ptr(df.binning), _ptr(df.img), _ptr(df.radii),
                                    _ptr(df.alpha), *[_ptr(u) for u in ups], *[_ptr(g[k]) for k in _GRAD_NAMES], _ptr(scratch),
                                    None, None, None, None)
        assert r >= 0, L.last_error()
        torch.cuda.synchronize()
    finally:
        L.set_option("bwd_records", before.get("bwd_records", 1))
    return {k: g[k].cpu().numpy() for k in _GRAD_NAMES}


def _chain_link(df, sc, up):
    """-> the outputs of the ordinary backward at bwd_records 0, checked against the dumped rows of the default blend"""
    fr = df.frame
    P, S, N = df.P, df.S, df.N
    out = df.blend(0, up)
    g = _raw_backward(df, sc, up, 0)
    count = np.bincount(fr.point_list.astype(np.int64), minlength=P)
    first = out["aux"][:, 0].astype(np.int64)
    listed = np.flatnonzero(count)
    order = listed[np.argsort(first[listed], kind="stable")]
    frm = RR.Frame(P, S, N, N, order.astype(np.uint32), first[order].astype(np.uint32), count.astype(np.uint32), out["flags"], 0)
    ref = RR.frame_reference(frm, RR.kernel_constants())
    exp = RR.expected_sums(ref, out["rows"][ref.slots])
    RR.check_arrays({k: g[k] for k in ("mean2D", "conic", "opacity", "color", "semantic", "depth")}, frm, ref, exp, 0, BR.row_floats(S))
    return g


@pytest.mark.parametrize("name", ["S10", "S17", "huge-64x48", "stack-129"])
def test_chain_link_rows_reduce_to_the_backward_outputs_bit_for_bit(name):
    """bwd_records 0: dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dsemantic and dL_ddepth of goi_raster_backward are the
    dumped rows added up in reduce_rows_k's order (tests/reduce_rows_reference.py), bit for bit."""
    (_name, sc, df, up), = _subset_cases((name,))
    _chain_link(df, sc, up)


# ---- every semantic width S = 1..32 (tests/channel_count_cases.py) ---------------------------------------------------------------
# The kernels above are compiled per S4 = ceil(S / 4) and take the 16-byte row path (LDS-DMA in the backward) for S % 4 == 0 only;
# the row cases of blend_cases.py reach S in {1, 3, 4, 10, 16, 17, 20, 32}.  One small frame per width -- two staging rounds,
# saturated and untouched pixels, ragged and empty quadrants (tests/test_channel_counts_cpu.py) -- through the same checks with
# the same tolerances.  The float32 yardstick over these 32 frames is part of the pooled GATE (docs/MEASUREMENT_LOG.md, "Every
# semantic width 1..32 through the frame kernels").
_WIDTH_FRAMES, _WIDTH_ROWS = {}, {}


def _width_case(S):
    """(tag, scene, frame, upstream gradients) of width S; the frames are small and kept for the module"""
    sc, _cam = CC.case(S)
    if S not in _WIDTH_FRAMES:
        _WIDTH_FRAMES[S] = DeviceFrame(sc, _cam, CC.BG)
    return f"width{S}", sc, _WIDTH_FRAMES[S], CC.upstream_dict(S)


def _width_default_rows(S):
    """the default backward rows of width S against the float64 reference: every element, validity byte and padded column;
    -> (normalised errors for the pooled gate, the yardstick's on the device's alphas); computed once per width"""
    if S not in _WIDTH_ROWS:
        tag, sc, df, up = _width_case(S)
        fr, qd = df.frame, df.quads
        out = df.blend(0, up)
        ref = BR.backward_rows(fr, qd, up, df.E, df.al, df.hit)
        slots = BR.slots_reference(fr, qd, out["aux"])
        BR.check_flags(slots, ref.member, out["flags"], df.N)
        ncol = BR.nsem_of(S) + 10
        got = np.zeros((qd.npairs, ncol), np.float32)
        got[ref.member] = _rows_of(out, slots[ref.member], ncol)
        err = BR.check_rows(S, qd, ref, got, BR.GATE, tag)
        y = BR.backward_rows(fr, qd, up, df.E, df.al, df.hit, dtype=np.float32)
        _WIDTH_ROWS[S] = (err, BR.normalised_errors(S, ref, y.rows)[0], int(ref.member.sum()), int(ref.depth.max()))
    return _WIDTH_ROWS[S]


@pytest.mark.parametrize("S", CC.WIDTHS)
def test_every_width_forward_and_default_backward_rows(S):
    """Pair evaluation of every candidate pair, qcost, member masks, n_contrib, out_alpha and the four maps, then slots, validity
    bytes and every element of every default-mode row, the padded semantic columns exactly 0."""
    tag, sc, df, up = _width_case(S)
    assert df.N > 0 and df.S == S
    fr, qd = df.frame, df.quads
    st = dict(N=df.N, pairs=qd.npairs, pair_eval=_check_pairs_chunked(fr, qd, df.E, df.al, df.guards))
    out = df.blend(0, up)
    BR.check_masks(qd, df.hit, out["qmask0"], out["qmask"], out["qcost"])
    assert (qd.qmax > 64).any() and (qd.nc.max(axis=1) < qd.length).any() and (~qd.inside).all(axis=1).any()
    st["forward"] = BR.check_forward(fr, qd, BR.forward_reference(fr, qd, df.al, df.hit), df.maps(), BR.GATE)
    err, _y, st["rows"], st["depth"] = _width_default_rows(S)
    st["kernel"] = {c: [x / BR.U for x in v[:3]] for c, v in BR.class_stats(S, err).items()}
    STATS[tag] = st
    print(tag, json.dumps(st, default=float), flush=True)


def test_every_width_default_rows_pass_the_pooled_gate():
    S_list = list(CC.WIDTHS)
    res = [_width_default_rows(S) for S in S_list]
    pooled = BR.pooled_stats(S_list, [r[0] for r in res])
    py = BR.pooled_stats(S_list, [r[1] for r in res])
    STATS["pooled/widths/kernel"] = {c: [x / BR.U for x in v[:3]] + [v[3]] for c, v in pooled.items()}
    STATS["pooled/widths/yardstick_device_alphas"] = {c: [x / BR.U for x in v[:3]] + [v[3]] for c, v in py.items()}
    print("pooled/widths", json.dumps({k: v for k, v in STATS.items() if k.startswith("pooled/widths")}, default=float), flush=True)
    BR.check_gate(pooled, BR.GATE, "every width, default mode: ")


@pytest.mark.parametrize("mode,what", OTHER_FORMS)
def test_other_forms_of_the_row_kernel_at_both_row_paths_of_every_S4(mode, what):
    """S = 4 S4 - 1 (rows through registers, one padded column) and 4 S4 (16-byte rows, LDS-DMA) for S4 = 1..8"""
    _other_form(mode, what, (_width_case(S) for S in CC.PAIRED_WIDTHS), f"pooled/widths/mode{mode}")


@pytest.mark.parametrize("S", CC.PAIRED_WIDTHS)
def test_semantic_only_rows_and_per_tile_kernel_at_both_row_paths_of_every_S4(S):
    """render_bwd_sem_k in its four forms (modes 4..7: either flush, member masks or candidate testing) and render_bwd_tile_k"""
    _semantic_only_rows([_width_case(S)], (4, 5, 6, 7))
    _per_tile_arrays([_width_case(S)])


@pytest.mark.parametrize("S", CC.WIDTHS)
def test_chain_link_and_record_paths_at_every_width(S):
    """The chain link at bwd_records 0, and the nine gradients the operator returns at bwd_records 1 (records in the row scratch:
    the default) and 2 (rows summed inside the per-Gaussian backward where a row has 32 floats, S = 5..20; the records elsewhere)
    equal to it element for element: the relation tests/test_gpu_parity.py asserts for these options on its own shapes.  (dL_dconic and
    dL_ddepth are inputs of the per-Gaussian backward that only the six-array path writes out.)"""
    _tag, sc, df, up = _width_case(S)
    g0 = _chain_link(df, sc, up)
    assert g0["semantic"].shape == (df.P, S) and np.isfinite(g0["semantic"]).all()
    for records in (1, 2):
        g = _raw_backward(df, sc, up, records)
        for k in ("mean2D", "color", "semantic", "opacity", "mean3D", "cov3D", "sh", "scale", "rot"):
            # (equality of VALUES, torch.equal's as in the parity suite: a zero gradient may leave either path as +0 or -0)
            assert np.isfinite(g[k]).all() and np.isfinite(g0[k]).all(), f"width {S}: dL_d{k} was not written everywhere"
            differ = g[k] != g0[k]
            assert not differ.any(), (f"width {S}: dL_d{k} at bwd_records {records} differs from 0 in {int(differ.sum())} elements, by up to "
                                      f"{float(np.abs(g[k].astype(np.float64) - g0[k])[differ].max()):.3e}")
