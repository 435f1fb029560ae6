"""goi_hyperplane_amd.pca (csrc/pca.hip) and the viewer's "semantics" mode on the GPU.

The fit is held to the float64 restatement (tests/pca_reference.py, itself held to sklearn's results by
tests/test_pca_cpu.py).  A case's tolerance is 8 x the error a float32 run of the reference has on that case (sklearn's
own float32 fit for the pinned cases, the restatement in float32 for the synthetic ones) with a floor of 64 float32 ulps of
the quantity's scale: max |x| for the mean, 1 for a unit component, the largest eigenvalue for the explained variances (an
eigenvalue moves by at most the norm of the covariance's error, whichever eigenvalue it is).  A component is compared
only where the reference's own eigenvalue is a factor 1.3 from both neighbours (and not float64 noise about zero): with
fewer samples than channels the trailing directions are degenerate and no two correct programs agree on them.  The normalised outputs are compared BIT
FOR BIT with the float32 restatement applied to the kernel's own raw projection and basis; a NaN matches a NaN.

Shapes: S in {3, 10, 16, 17, 32} (the padded 16 x 16 block, the full one, one and two channels into the second) and
n in {2, 3, 63, 64, 65, 255, 257, 4099, 70001} (the tail of a wave, n % 4 through all its values, more groups than one
pass of the fixed grid), both layouts."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests import pca_reference as ref

pytestmark = pytest.mark.gpu

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pca_pins.npz")
DIMS = [3, 10, 16, 17, 32]
COUNTS = [2, 3, 63, 64, 65, 255, 257, 4099, 70001]
ULPS = 64 * ref.EPS32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pins():
    with np.load(PINS) as z:
        return {k: z[k] for k in z.files}


def gpu_rows(dev, rows, layout):
    """The samples on the device in `layout`: rows [n, S] as they are, planar as the [S, n] transpose."""
    a = rows if layout == "rows" else np.ascontiguousarray(rows.T)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def download(basis):
    d = basis.data.cpu().numpy()
    S = basis.S
    return ref.Basis(d[:S], d[S:4 * S].reshape(3, S), d[4 * S:4 * S + 3], d[4 * S + 3], d[4 * S + 4])


def separated(rows, mask=None):
    """Which of the three components the reference itself determines: eigenvalue ratios of >= 1.3 to both neighbours."""
    with np.errstate(all="ignore"):
        w = np.maximum(ref.eigenvalues(rows, mask), 0)
        w[w < 1e-12 * w[0]] = 0  # below float64's own noise on this matrix: the sample has no such direction
        ok = []
        for k in range(3):
            below = True if k + 1 >= len(w) else w[k] / w[k + 1] >= 1.3
            above = True if k == 0 else w[k - 1] / w[k] >= 1.3
            ok.append(bool(below and above and w[k] > 0))
    return ok


def recorded_error(rows, mask=None):
    """(mean, components, explained variance relative to the largest) of the restatement run in float32."""
    a, b = ref.fit(rows, mask), ref.fit(rows, mask, np.float32)
    sep = separated(rows, mask)
    comp = max([np.abs(a.components[k] - b.components[k].astype(np.float64)).max() for k in range(3) if sep[k]], default=0.0)
    return (np.abs(a.mean - b.mean).max(), comp, np.abs(a.explained_variance - b.explained_variance).max() / a.explained_variance[0])


def check_fit(got, rows, mask=None, err32=None, what=""):
    want = ref.fit(rows, mask)
    used = rows if mask is None else rows[np.asarray(mask).reshape(-1) != 0]
    e_mean, e_comp, e_ev = recorded_error(rows, mask) if err32 is None else err32
    tol_mean = max(8 * e_mean, ULPS * float(np.abs(used).max()))
    tol_comp = max(8 * e_comp, ULPS)
    tol_ev = max(8 * e_ev, ULPS)
    sep = separated(rows, mask)
    d_mean = np.abs(got.mean - want.mean).max()
    d_ev = np.abs(got.explained_variance - want.explained_variance).max() / want.explained_variance[0]
    d_tot = abs(got.total_variance - want.total_variance) / want.explained_variance[0]
    d_comp = max([np.abs(got.components[k] - want.components[k]).max() for k in range(3) if sep[k]], default=0.0)
    print(f"pca fit {what}: mean {d_mean:.2e} / {tol_mean:.2e}  ev {d_ev:.2e} / {tol_ev:.2e}  total {d_tot:.2e}  "
          f"components {d_comp:.2e} / {tol_comp:.2e}  compared {sep}")
    assert got.count == want.count, what
    assert np.isfinite(np.concatenate([got.mean, got.components.ravel(), got.explained_variance])).all(), what
    assert d_mean <= tol_mean and d_ev <= tol_ev and d_comp <= tol_comp, what
    assert d_tot <= len(want.mean) * tol_ev, what  # a sum of S eigenvalues
    assert (np.diff(got.explained_variance) <= 0).all() and (got.explained_variance >= 0).all(), what
    for k in range(3):
        if sep[k]:
            assert got.components[k, np.argmax(np.abs(got.components[k]))] > 0, (what, k)
    return tol_mean, tol_comp, tol_ev


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, int(bad.sum()), "first at", np.argwhere(bad)[0].tolist())


# ---- 1. the fit against the float64 reference --------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["planar", "rows"])
@pytest.mark.parametrize("S", DIMS)
def test_fit_matches_the_float64_reference(dev, S, layout):
    from goi_hyperplane_amd import pca
    for n in COUNTS:
        rows = ref.sample(S, n, seed=1000 * S + n)
        b = pca.fit(gpu_rows(dev, rows, layout), layout=layout)
        assert b.S == S and b.data.shape == (4 * S + 5,)
        check_fit(download(b), rows, what=f"S={S} n={n} {layout}")


@pytest.mark.parametrize("layout", ["planar", "rows"])
def test_fit_matches_sklearn_pins(dev, pins, layout):
    from goi_hyperplane_amd import pca
    for name in ("s3", "s10", "s16", "s17", "s32"):
        x = pins[name + "_x"]
        got = download(pca.fit(gpu_rows(dev, x, layout), layout=layout))
        e = pins[name + "_err32"]
        check_fit(got, x, err32=(e[0], e[1], e[2]), what=f"{name} {layout}")
        assert np.abs(got.components - pins[name + "_components"]).max() <= max(8 * e[1], ULPS), name
        big = np.abs(pins[name + "_components"]) > max(8 * e[1], ULPS)  # an entry inside the tolerance has no sign to compare
        assert np.array_equal(np.sign(got.components)[big], np.sign(pins[name + "_components"])[big]), name


# ---- 2. features far from zero: the tolerance of the same data without the offset ---------------------------------------
@pytest.mark.parametrize("layout", ["planar", "rows"])
def test_offset_by_100_sigma_keeps_the_tolerance(dev, pins, layout):
    from goi_hyperplane_amd import pca
    e = pins["s16_err32"]
    x = pins["s16_offset_x"]
    assert (np.abs(x.mean(0)) / x.std(0)).min() > 90
    check_fit(download(pca.fit(gpu_rows(dev, x, layout), layout=layout)), x, err32=(e[0], e[1], e[2]), what=f"pinned offset {layout}")
    for S, n in ((10, 4099), (32, 70001), (17, 257)):
        plain, moved = ref.sample(S, n, seed=77 + S), ref.sample(S, n, seed=77 + S, offset=100.0)
        assert (np.abs(moved.mean(0)) / moved.std(0)).min() > 90
        got = download(pca.fit(gpu_rows(dev, moved, layout), layout=layout))
        # the mean's floor is that of the data it is the mean of: |x| is now ~100 sigma and so is its float32 grid
        check_fit(got, moved, err32=recorded_error(plain), what=f"offset S={S} n={n} {layout}")


@pytest.mark.parametrize("S,H,W", [(10, 64, 64), (16, 96, 128), (32, 40, 52)])
def test_offset_foreground_under_an_empty_first_block(dev, S, H, W):
    """What the viewer fits: the first rows of the map are empty background (zeros) that the mask excludes, the foreground
    below sits 100 sigma from zero.  A pivot taken from the first samples would be the background's value and leave the
    raw moments; the tolerance is that of the foreground's samples WITHOUT the offset."""
    from goi_hyperplane_amd import pca
    top = (H // 2) * W  # far more than the 2048 samples a pivot looks at
    n_fg = H * W - top
    plain, moved = ref.sample(S, n_fg, seed=S + H), ref.sample(S, n_fg, seed=S + H, offset=100.0)
    rows = np.concatenate([np.zeros((top, S), np.float32), moved])
    m = np.arange(H * W) >= top
    x = torch.from_numpy(np.ascontiguousarray(rows.T)).to(dev).reshape(S, H, W)
    mask = torch.from_numpy(m).to(dev).reshape(H, W)
    check_fit(download(pca.fit(x, mask=mask)), moved, err32=recorded_error(plain), what=f"empty first block S={S} {H}x{W}")
    xr = torch.from_numpy(rows).to(dev)
    check_fit(download(pca.fit(xr, layout="rows", mask=mask)), moved, err32=recorded_error(plain), what=f"empty first block S={S} rows")
    # and over several views whose FIRST is the one with the empty block
    b = pca.fit_views([x, x], [mask, mask])
    check_fit(download(b), np.concatenate([moved, moved]), err32=recorded_error(plain), what=f"empty first block S={S} two views")


# ---- 3. masks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["planar", "rows"])
@pytest.mark.parametrize("S,n", [(16, 4099), (32, 257), (10, 70001), (3, 64)])
def test_mask_selects_the_samples(dev, S, n, layout):
    from goi_hyperplane_amd import pca
    rows = ref.sample(S, n, seed=5 * S + n)
    m = np.random.default_rng(S + n).uniform(size=n) < 0.4
    x = gpu_rows(dev, rows, layout)
    for mask in (torch.from_numpy(m).to(dev), torch.from_numpy(m.astype(np.uint8) * 7).to(dev)):
        check_fit(download(pca.fit(x, layout=layout, mask=mask)), rows[m], what=f"mask S={S} n={n} {layout} {mask.dtype}")
    ones = download(pca.fit(x, layout=layout, mask=torch.ones(n, dtype=torch.bool, device=dev)))
    tol_mean, tol_comp, tol_ev = check_fit(ones, rows, what=f"all-ones mask S={S} n={n} {layout}")
    none = download(pca.fit(x, layout=layout))
    assert np.abs(ones.mean - none.mean).max() <= tol_mean and np.abs(ones.components - none.components).max() <= tol_comp
    assert np.abs(ones.explained_variance - none.explained_variance).max() <= tol_ev * none.explained_variance[0]


# ---- 4. several views into one workspace -----------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [10, 32])
def test_fit_views_is_one_fit_of_the_concatenation(dev, S):
    from goi_hyperplane_amd import pca
    shapes = [(16, 24), (7, 9), (33, 65)]
    rows = ref.sample(S, sum(h * w for h, w in shapes), seed=31 + S)
    maps, at = [], 0
    for h, w in shapes:
        maps.append(torch.from_numpy(np.ascontiguousarray(rows[at:at + h * w].T)).to(dev).reshape(S, h, w))
        at += h * w
    b = pca.fit_views(maps)
    check_fit(download(b), rows, what=f"fit_views S={S}")
    m = np.random.default_rng(S).uniform(size=len(rows)) < 0.4
    masks, at = [], 0
    for h, w in shapes:
        masks.append(torch.from_numpy(m[at:at + h * w]).to(dev).reshape(h, w))
        at += h * w
    check_fit(download(pca.fit_views(maps, masks)), rows[m], what=f"fit_views masked S={S}")
    # first = 1, 0, 0 on a workspace that holds another fit: nothing of it survives
    f = pca.Fit(S, dev)
    junk = torch.from_numpy(ref.sample(S, 5000, seed=9, offset=30.0).T.copy()).to(dev)
    f.add(junk).add(junk)
    f.reset()
    for x in maps:
        f.add(x)
    assert f.calls == 3 and torch.equal(f.solve().data.view(torch.int32), b.data.view(torch.int32))


# ---- 5. the projection and its normalisations ------------------------------------------------------------------------------
def batch_of_views(S, H, W, seed):
    """Three views whose ranges are far apart."""
    return np.stack([ref.sample(S, H * W, seed + v).T.reshape(S, H, W) * sc + off
                     for v, (sc, off) in enumerate(((1.0, 0.0), (100.0, 30.0), (0.01, -2.0)))]).astype(np.float32)


def check_normalisations(dev, x, basis, what, k=2.0):
    """x [V, S, H, W] float32 numpy: RAW against the float64 projection with the kernel's own basis, SIGMA and MINMAX bit for
    bit against the restatement on the kernel's own RAW q."""
    from goi_hyperplane_amd import pca
    V, S, H, W = x.shape
    t = torch.from_numpy(x).to(dev)
    b = download(basis)
    q = pca.transform(t, basis, normalize="raw")
    assert q.shape == (V, 3, H, W)
    q = q.cpu().numpy()
    for v in range(V):
        rows = x[v].reshape(S, -1).T
        q64 = ref.project(rows, b)
        q32 = ((rows - b.mean) @ b.components.T).astype(np.float32)  # the projection in float32: the recorded error
        finite = np.isfinite(q64).all(axis=1)
        scale = np.abs(q64[finite]).max()
        tol = max(8 * np.abs(q32[finite] - q64[finite]).max(), ULPS * scale)
        got = q[v].reshape(3, -1).T
        d = np.abs(got[finite] - q64[finite]).max()
        print(f"pca project {what} view {v}: {d:.2e} / {tol:.2e}")
        assert d <= tol and np.isnan(got[~finite]).all(), (what, v)
    sig = pca.transform(t, basis, normalize="sigma", k_sigma=k)
    mm = pca.transform(t, basis, normalize="minmax")
    for v in range(V):
        qv = q[v].reshape(3, -1).T
        same_bits(sig[v].cpu().numpy().reshape(3, -1).T, ref.sigma(qv, b.explained_variance, k), (what, "sigma", v))
        same_bits(mm[v].cpu().numpy().reshape(3, -1).T, ref.minmax(qv), (what, "minmax", v))
    s = sig.cpu().numpy()
    assert (s >= 0).all() and (s <= 1).all()
    # one view alone is the same as that view in the batch (each has its own minimum and maximum)
    for mode, batch in (("sigma", sig), ("minmax", mm)):
        one = pca.transform(t[V - 1], basis, normalize=mode, k_sigma=k)
        assert one.shape == (3, H, W)
        same_bits(one, batch[V - 1].cpu().numpy(), (what, mode, "single view"))
    return q, sig, mm


@pytest.mark.parametrize("S", DIMS)
@pytest.mark.parametrize("H,W", [(16, 24), (7, 9), (5, 13), (1, 2)])
def test_normalisations_equal_the_restatement_bit_for_bit(dev, S, H, W):
    """16 x 24: the vector path; 7 x 9, 5 x 13, 1 x 2: n % 4 = 3, 1, 2, every view after the first misaligned."""
    from goi_hyperplane_amd import pca
    x = batch_of_views(S, H, W, seed=S + H)
    basis = pca.fit(torch.from_numpy(ref.sample(S, 3000, seed=S).T.copy()).to(dev))
    check_normalisations(dev, x, basis, f"S={S} {H}x{W}")
    check_normalisations(dev, x, basis, f"S={S} {H}x{W} k=0.75", k=0.75)


@pytest.mark.parametrize("H,W", [(16, 24), (7, 9)])
def test_a_nan_feature_and_a_constant_view(dev, H, W):
    from goi_hyperplane_amd import pca
    S = 10
    x = batch_of_views(S, H, W, seed=3)
    x[0, 4, H // 2, W // 3] = np.nan  # ONE feature of one pixel
    x[1] = 0.5  # a constant view
    basis = pca.fit(torch.from_numpy(ref.sample(S, 3000, seed=S).T.copy()).to(dev))
    q, sig, mm = check_normalisations(dev, x, basis, f"nan + constant {H}x{W}")
    assert np.isnan(q[0, :, H // 2, W // 3]).all() and np.isnan(q[0]).sum() == 3
    assert (sig[0, :, H // 2, W // 3] == 0).all() and torch.isnan(mm[0, :, H // 2, W // 3]).all()
    m0 = mm[0].cpu().numpy()
    assert np.nanmin(m0) == 0 and np.nanmax(m0) == 1 and np.isnan(m0).sum() == 3  # the NaN was skipped, not spread
    assert not mm[1].any()  # range 0 gives 0
    # a basis fitted on the constant view itself: sigma = 0 gives 0.5, and nothing is NaN
    flat = pca.fit(torch.from_numpy(x[1]).to(dev))
    b = download(flat)
    # (the components of a zero covariance are arbitrary unit vectors, as sklearn's are: only their variance is pinned)
    assert not b.explained_variance.any() and b.total_variance == 0 and b.count == H * W
    assert np.array_equal(b.mean, np.full(S, 0.5, np.float32)) and np.isfinite(b.components).all()
    assert (pca.transform(torch.from_numpy(x[1]).to(dev), flat, normalize="sigma") == 0.5).all()
    assert not pca.transform(torch.from_numpy(x[1]).to(dev), flat, normalize="minmax").any()


# ---- 6. layouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n", [(16, 4096), (17, 255), (32, 4099), (3, 65)])
def test_layouts_agree(dev, S, n):
    from goi_hyperplane_amd import pca
    rows = ref.sample(S, n, seed=S * n)
    xp, xr = gpu_rows(dev, rows, "planar"), gpu_rows(dev, rows, "rows")
    bp, br = pca.fit(xp, layout="planar"), pca.fit(xr, layout="rows")
    tol_mean, tol_comp, tol_ev = check_fit(download(bp), rows, what=f"layouts S={S} n={n} planar")
    check_fit(download(br), rows, what=f"layouts S={S} n={n} rows")
    p, r = download(bp), download(br)
    assert np.abs(p.mean - r.mean).max() <= tol_mean and np.abs(p.components - r.components).max() <= tol_comp
    for mode in ("raw", "sigma", "minmax"):
        planar = pca.transform(xp, bp, normalize=mode)  # [3, n]
        as_rows = pca.transform(xp, bp, normalize=mode, out_layout="rows")  # [n, 3]
        assert planar.shape == (3, n) and as_rows.shape == (n, 3)
        same_bits(as_rows, planar.cpu().numpy().T.copy(), (mode, "output layouts"))
        from_rows = pca.transform(xr, bp, layout="rows", normalize=mode)  # the same samples, the other input layout
        assert from_rows.shape == (n, 3)
        same_bits(from_rows, as_rows.cpu().numpy(), (mode, "input layouts"))
        same_bits(pca.transform(xr, bp, layout="rows", normalize=mode, out_layout="planar"), planar.cpu().numpy(), (mode, "rows -> planar"))
        out = torch.empty_like(planar)
        assert pca.transform(xp, bp, normalize=mode, out=out) is out
        same_bits(out, planar.cpu().numpy(), (mode, "out="))


# ---- 7. reproducibility ----------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits(dev):
    from goi_hyperplane_amd import pca
    for S, n, layout in ((16, 70001, "planar"), (32, 70000, "planar"), (10, 4099, "rows")):
        rows = ref.sample(S, n, seed=S)
        x = gpu_rows(dev, rows, layout)
        m = torch.from_numpy(np.random.default_rng(n).uniform(size=n) < 0.5).to(dev)
        runs = []
        for _ in range(2):
            b = pca.fit(x, layout=layout, mask=m)
            runs.append((b.data.clone(), pca.transform(x, b, layout=layout, normalize="minmax"), pca.transform(x, b, layout=layout, normalize="sigma")))
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_fit_and_transform_never_synchronise(dev):
    from goi_hyperplane_amd import pca
    x = gpu_rows(dev, ref.sample(16, 4096, seed=2), "planar").reshape(16, 64, 64)
    m = torch.ones(64, 64, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = pca.fit_views([x, x], [m, None])
        for mode in ("raw", "sigma", "minmax"):
            pca.transform(x, b, normalize=mode)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert float(b.count) == 8192


# ---- 8. fewer than two samples ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 16, 32])
def test_fewer_than_two_samples(dev, S):
    from goi_hyperplane_amd import pca
    rows = ref.sample(S, 40, seed=S)
    one = download(pca.fit(gpu_rows(dev, rows[:1], "rows"), layout="rows"))
    assert one.count == 1 and not one.components.any() and not one.explained_variance.any() and one.total_variance == 0
    assert np.abs(one.mean - rows[0]).max() <= ULPS * np.abs(rows[0]).max()
    x = gpu_rows(dev, rows, "planar").reshape(S, 5, 8)
    for used in (0, 1):
        m = torch.zeros(40, dtype=torch.bool, device=dev)
        m[17:17 + used] = True
        basis = pca.fit(x, mask=m)
        b = download(basis)
        assert b.count == used and not b.components.any() and not b.explained_variance.any()
        assert np.isfinite(basis.data.cpu().numpy()).all()
        if used:
            assert np.abs(b.mean - rows[17]).max() <= ULPS * np.abs(rows[17]).max()
        for mode in ("raw", "sigma", "minmax"):
            frame = pca.transform(x, basis, normalize=mode)
            assert torch.isfinite(frame).all(), (used, mode)
        assert (pca.transform(x, basis, normalize="sigma") == 0.5).all()


# ---- 9. the viewer ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(dev):
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import make_camera, make_scene
    from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, svm_score_fn
    pc = GaussianSet.from_scene(make_scene(P=2000, S=10), dev)
    cams = [TorchCamera(make_camera(64, 48, yaw=y, distance=5.0), dev) for y in (0.0, 0.7, 2.1)]
    torch.manual_seed(3)
    mlp = SemanticModel(dim_in=10, dim_out=4, num_layer=1, use_bias=True, device=dev)
    u = torch.nn.functional.normalize(torch.randn(256, device=dev), dim=0)
    lut = torch.stack([u, -u, u, -u]) + 0.01 * torch.randn(4, 256, device=dev)
    svm = LinearSVM().to(dev)
    svm.weight_set(u.reshape(1, -1))
    table = torch.from_numpy(np.random.default_rng(5).uniform(0, 1, (256, 3)).astype(np.float32)).to(dev)
    return pc, mlp, lut, svm_score_fn(svm), cams, table


def bits_equal(a, b):
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("style", ["none", "heat"])
def test_view_frame_semantics_is_compose_of_transform(dev, scene, style):
    from goi_hyperplane_amd import display, pca
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import view_frame
    pc, mlp, lut, score_fn, cams, table = scene
    bgc = torch.zeros(3, device=dev)
    out = render_gui(cams[0], pc, bgc)
    sem = out["semantics"]
    assert sem.shape == (10, 48, 64) and float(sem.abs().max()) > 0
    for dtype in (torch.float32, torch.uint8):
        for kw, basis, normalize in (({}, pca.fit(sem), "sigma"),
                                     (dict(pca_mask_alpha=0.5), pca.fit(sem, mask=out["alpha"].reshape(-1) > 0.5), "sigma"),
                                     (dict(pca_normalize="minmax"), pca.fit(sem), "minmax"),
                                     (dict(basis=pca.fit_gaussians(pc)), pca.fit_gaussians(pc), "sigma")):
            frame, parts = view_frame(cams[0], pc, mlp, lut, score_fn, 0.5, bgc, mode="semantics", style=style, overlay_ratio=0.6,
                                      dtype=dtype, colormap=table, return_parts=True, **kw)
            base = pca.transform(sem, basis, normalize=normalize)
            assert frame.shape == (48, 64, 3) and frame.dtype == dtype and bits_equal(parts["base"], base)
            want = display.compose(base, parts["sim"], parts["bg_mask"], style=style, overlay_ratio=0.6, colormap=table, dtype=dtype)
            assert bits_equal(frame, want), (style, dtype, kw.keys())
            assert (parts["sim"] is None) == (style == "none")
    assert float(frame.float().std()) > 0  # a picture, not a flat field


def test_video_frames_semantics(dev, scene):
    from goi_hyperplane_amd import display, pca
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import video_frames, view_frame
    pc, mlp, lut, score_fn, cams, table = scene
    bgc = torch.zeros(3, device=dev)
    sems = [render_gui(c, pc, bgc)["semantics"].clone() for c in cams]
    # no basis: ONE basis over the whole camera set
    shared = pca.fit_views(sems)
    frames = video_frames(cams, pc, mlp, lut, score_fn, 0.5, bgc, mode="semantics", style="none", dtype=torch.float32)
    assert frames.shape == (3, 48, 64, 3)
    want = display.compose(torch.stack([pca.transform(s, shared, normalize="sigma") for s in sems]), style="none")
    assert bits_equal(frames, want)
    # a given basis: every frame is view_frame's with that basis
    given = pca.fit_gaussians(pc)
    for style, dtype in (("heat", torch.uint8), ("none", torch.float32)):
        frames = video_frames(cams, pc, mlp, lut, score_fn, 0.5, bgc, mode="semantics", style=style, overlay_ratio=0.6, dtype=dtype,
                              colormap=table, basis=given)
        for v, cam in enumerate(cams):
            single = view_frame(cam, pc, mlp, lut, score_fn, 0.5, bgc, mode="semantics", style=style, overlay_ratio=0.6, dtype=dtype,
                                colormap=table, basis=given)
            assert bits_equal(frames[v], single), (style, v)
    assert not torch.equal(frames[0], frames[1])
    # with one basis a pixel's colour depends on its feature alone: two views that share a feature map
    both = pca.transform(torch.stack([sems[0], sems[0], sems[1]]), given, normalize="sigma")
    assert bits_equal(both[0], both[1]) and bits_equal(both[0], pca.transform(sems[0], given, normalize="sigma"))
    flat = sems[0].reshape(10, -1)
    perm = torch.randperm(flat.shape[1], device=dev)
    moved = pca.transform(flat[:, perm].contiguous(), given, normalize="sigma")
    assert bits_equal(moved, both[0].reshape(3, -1)[:, perm].contiguous())


@pytest.mark.parametrize("mode", ["image", "depth", "alpha"])
def test_the_other_modes_are_untouched(dev, scene, mode):
    from goi_hyperplane_amd import display
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import video_frames, view_frame
    pc, mlp, lut, score_fn, cams, table = scene
    bgc = torch.zeros(3, device=dev)
    for style in ("none", "heat"):
        frame, parts = view_frame(cams[0], pc, mlp, lut, score_fn, 0.5, bgc, mode=mode, style=style, colormap=table, return_parts=True)
        out = render_gui(cams[0], pc, bgc)
        base = out[mode].reshape((-1, 48, 64))
        assert bits_equal(parts["base"], base)
        want = display.compose(base, parts["sim"], parts["bg_mask"], style=style, normalize=mode == "depth", colormap=table)
        assert bits_equal(frame, want), (mode, style)
        frames = video_frames(cams, pc, mlp, lut, score_fn, 0.5, bgc, mode=mode, style=style, colormap=table, dtype=torch.float32)
        assert bits_equal(frames[0], frame), (mode, style)


def test_semantics_mode_refuses_bad_arguments(dev, scene):
    from goi_hyperplane_amd.semantic import view_frame
    pc, mlp, lut, score_fn, cams, table = scene
    bgc = torch.zeros(3, device=dev)
    with pytest.raises(ValueError, match="pca_normalize"):
        view_frame(cams[0], pc, mlp, lut, score_fn, 0.5, bgc, mode="semantics", style="none", pca_normalize="zscore")
    with pytest.raises(TypeError, match="PcaBasis"):
        view_frame(cams[0], pc, mlp, lut, score_fn, 0.5, bgc, mode="semantics", style="none", basis=torch.zeros(45, device=dev))
    with pytest.raises(ValueError, match="mode must be one of"):
        view_frame(cams[0], pc, mlp, lut, score_fn, 0.5, bgc, mode="features", style="none")


# ---- 10. the Gaussians' own colours -----------------------------------------------------------------------------------------
def test_gaussian_colors_render(dev, scene):
    from goi_hyperplane_amd import pca
    from goi_hyperplane_amd.render import render_gui
    pc, mlp, lut, score_fn, cams, table = scene
    colors = pca.gaussian_colors(pc)
    sem = pc.get_semantics.detach()
    assert colors.shape == (2000, 3) and colors.dtype == torch.float32
    assert float(colors.min()) >= 0 and float(colors.max()) <= 1 and float(colors.std()) > 0.05
    basis = pca.fit_gaussians(pc)
    assert bits_equal(colors, pca.transform(sem, basis, layout="rows", normalize="sigma"))
    check_fit(download(basis), sem.cpu().numpy(), what="fit_gaussians")
    mm = pca.gaussian_colors(pc, basis, normalize="minmax")
    assert bits_equal(mm, pca.transform(sem, basis, layout="rows", normalize="minmax")) and float(mm.min()) == 0 and float(mm.max()) <= 1
    with pytest.raises(ValueError, match="not colours"):
        pca.gaussian_colors(pc, normalize="raw")
    out = render_gui(cams[0], pc, torch.zeros(3, device=dev), override_color=colors)
    img = out["image"]
    assert img.shape == (3, 48, 64) and torch.isfinite(img).all() and float(img.max()) > 0
    plain = render_gui(cams[0], pc, torch.zeros(3, device=dev))["image"]
    assert not torch.equal(img, plain)
