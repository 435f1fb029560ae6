"""goi_hyperplane_amd.field (csrc/field.hip) on the GPU: the density grid, the iso-surface and extract_mesh.

Density.  Every grid point is compared with the float64 restatement (tests/field_reference.py: density_f64), none excluded.
The error is relative to |value| + 64 float32 ulps of the point's sum of member opacities; a case's gate is 8 x the error
the float32 torch restatement of the reference's own block loop (density_f32_reference: gaussian_3d_coeff per pair as
written, batches of 1024) has on the same case -- summation order and the device's exp differ from torch's.  That
reference error was confirmed small on the CPU when the cases were written (1e-6 .. 3e-4).  Grids: R = 16 / 2 blocks
(split 8), R = 24 / 6 blocks (split 4), R = 32 / 2 blocks (split 16); the per-block member counts reach 0, 1, BATCH - 1,
BATCH, BATCH + 1 and 3 BATCH + 7 of the kernel's LDS batch (field.BATCH); anisotropy up to 10 : 1, normalised scales from
0.02, opacities on both sides of 0.005 and one exactly 0.005, centres exactly on a widened block bound, a NaN and an infinite
centre, a selection and its inverse, a `bounds` override.

Measured on an MI355X, max over the grid of the device's error / the float32 reference's error = ratio, occ (attr alike):
    clusters24 9.9e-7 / 4.7e-6 = 0.21   clusters24_sel 7.7e-7 / 8.9e-7 = 0.87   clusters24_inv 9.9e-7 / 4.7e-6 = 0.21
    random16 1.3e-5 / 3.1e-5 = 0.40   clusters32 1.1e-5 / 6.7e-5 = 0.16   random32 2.7e-5 / 3.5e-5 = 0.79
    batch16 1.2e-5 / 3.2e-5 = 0.38   random24 2.4e-5 / 5.2e-5 = 0.45
(the reference's figure depends on the host: its bmm rounds the covariance differently from machine to machine, 3.0e-4 or
3.5e-5 on random32.  The kernel forms the inverse covariance in fp64 once per Gaussian, which is why it stays below.)

Iso-surface.  On analytic grids uploaded from the host, `faces` are integer-equal and `vertices` / `colors` bit-equal to
the float32 numpy restatement (marching_tets): the device's division is IEEE and the unit is compiled without contraction,
so no ulp allowance is needed.

End to end.  extract_mesh on 2000 Gaussians on a sphere shell at R = 32."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from tests import field_reference as ref

pytestmark = pytest.mark.gpu

MARGIN = 8  # the margin of the PCA stage's gate
UNIT = (np.zeros(3, np.float32), 1.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def B():
    from goi_hyperplane_amd import field
    return field.BATCH


def specs():
    b = B()
    return {
        "clusters24": dict(R=24, nb=6, relax=0.25, kind="cluster", seed=1, bounds=UNIT,
                           counts={(0, 0, 0): 1, (1, 2, 3): b - 1, (5, 5, 5): b, (3, 0, 4): b + 1, (2, 4, 1): 3 * b + 7}),
        "clusters24_sel": dict(base="clusters24", select=False),
        "clusters24_inv": dict(base="clusters24", select=True),
        "random16": dict(R=16, nb=2, relax=1.5, kind="random", P=300, seed=2),
        "clusters32": dict(R=32, nb=2, relax=0.25, kind="cluster", seed=3, bounds=UNIT,
                           counts={(0, 1, 0): b + 1, (1, 0, 1): 3 * b + 7, (1, 1, 1): 1}),
        "random32": dict(R=32, nb=2, relax=1.5, kind="random", P=3 * b + 7 + 8, seed=4),
        "batch16": dict(R=16, nb=2, relax=1.5, kind="random", P=b + 8, seed=6),
        "random24": dict(R=24, nb=6, relax=1.5, kind="random", P=300, seed=2),
    }


CASES = ["clusters24", "clusters24_sel", "clusters24_inv", "random16", "clusters32", "random32", "batch16", "random24"]


@functools.lru_cache(maxsize=None)
def device_coords(R):
    return torch.linspace(-1, 1, R, dtype=torch.float32, device="cuda:0").cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, model, kwargs of the restatements, float64 truth, float32 reference error (occ, attr)) -- computed once."""
    s = dict(specs()[name])
    kw = {}
    if "base" in s:
        base = dict(specs()[s["base"]])
        model = case(s["base"])[1]
        sel = np.random.default_rng(5).random(len(model["opacity"])) < 0.5
        kw = dict(selection=sel, selection_invert=s["select"])
        s = {**base, **s}
    elif s["kind"] == "cluster":
        model = ref.cluster_case(device_coords(s["R"]), s["R"], s["nb"], s["relax"], s["counts"], s["seed"])
    else:
        model = ref.random_case(s["P"], s["seed"])
    if s.get("bounds") is not None:
        kw["bounds"] = s["bounds"]
    kw["coords"] = device_coords(s["R"])
    truth = ref.density_f64(model, s["R"], s["nb"], s["relax"], attributes=model["rgb"], **kw)
    o32, a32 = ref.density_f32_reference(model, s["R"], s["nb"], s["relax"], attributes=model["rgb"], **kw)
    err = (ref.relative_error(o32, truth["occ"], truth["opsum"]), ref.relative_error(a32, truth["attr"], truth["opsum"][None]))
    return s, model, kw, truth, err


def run_density(dev, s, model, kw, attributes=True, **over):
    from goi_hyperplane_amd import field
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    args = dict(resolution=s["R"], num_blocks=s["nb"], relax_ratio=s["relax"])
    if "selection" in kw:
        args.update(selection=t(kw["selection"]), selection_invert=kw["selection_invert"])
    if "bounds" in kw:
        args["bounds"] = (t(kw["bounds"][0]), torch.tensor(float(kw["bounds"][1]), device=dev))
    if attributes:
        args["attributes"] = t(model["rgb"])
    args.update(over)
    return field.density_grid(t(model["xyz"]), t(model["opacity"]), t(model["scaling"]), t(model["rotation"]), **args)


# ---- density ----------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_every_batch_edge():
    b = B()
    seen = set()
    for name in CASES:
        seen |= set(case(name)[3]["members"].ravel().tolist())
    assert {0, 1, b - 1, b, b + 1, 3 * b + 7} <= seen, sorted(seen)
    model = case("clusters24")[1]
    assert (model["opacity"] == np.float32(0.005)).sum() == 1 and (model["opacity"] < 0.005).sum() >= 5
    assert np.isnan(model["xyz"]).any() and np.isinf(model["xyz"]).any()
    _, lo, hi = ref.grid_tables(24, 6, 0.25, device_coords(24))
    assert (model["xyz"][:, 0] == lo[0]).sum() == 1 and (model["xyz"][:, 1] == hi[5]).sum() == 1
    for name in CASES:  # the float32 reference alone stays small: the cases can arbitrate
        assert max(case(name)[4]) < 1e-3, (name, case(name)[4])


@pytest.mark.parametrize("name", CASES)
def test_density_matches_float64(dev, name):
    s, model, kw, truth, (err_occ, err_attr) = case(name)
    f = run_density(dev, s, model, kw)
    occ, attr = f.occ.cpu().numpy(), f.attr.cpu().numpy()
    assert occ.shape == (s["R"],) * 3 and attr.shape == (3,) + (s["R"],) * 3 and int(f.status) == 0
    assert np.array_equal(f.center.cpu().numpy(), truth["center"]) and np.float32(f.scale.item()) == truth["scale"]
    assert np.array_equal(f.coords.cpu().numpy(), truth["coords"])
    d_occ = ref.relative_error(occ, truth["occ"], truth["opsum"])
    d_attr = ref.relative_error(attr, truth["attr"], truth["opsum"][None])
    print(f"\n{name}: device {d_occ:.3g} / {d_attr:.3g}  float32 reference {err_occ:.3g} / {err_attr:.3g}  "
          f"ratio {d_occ / max(err_occ, 1e-300):.2f} / {d_attr / max(err_attr, 1e-300):.2f}  max occ {truth['occ'].max():.3g}")
    assert d_occ <= MARGIN * err_occ, (d_occ, err_occ)
    assert d_attr <= MARGIN * err_attr, (d_attr, err_attr)
    assert np.all(occ[truth["opsum"] == 0] == 0)  # a point of a block without members is exactly zero


@pytest.mark.parametrize("name", ["clusters24", "random32"])
def test_density_is_reproducible_and_the_plain_kernel_agrees(dev, name):
    s, model, kw, _truth, _ = case(name)
    a, b = run_density(dev, s, model, kw), run_density(dev, s, model, kw)
    assert torch.equal(a.occ, b.occ) and torch.equal(a.attr, b.attr)
    plain = run_density(dev, s, model, kw, attributes=False)  # the instantiation without attribute channels: the same sums
    assert plain.attr is None and torch.equal(plain.occ, a.occ)


def test_selection_in_place_equals_the_gathered_model(dev):
    """The members of a block keep their relative order under index selection, so the sums are the same bits."""
    s, model, kw, _truth, _ = case("clusters24_sel")
    sel = kw["selection"] != kw["selection_invert"]
    f = run_density(dev, s, model, kw)
    gathered = {k: v[sel] for k, v in model.items()}
    g = run_density(dev, s, gathered, {"bounds": kw["bounds"]})
    assert torch.equal(f.occ, g.occ) and torch.equal(f.attr, g.attr)
    u8 = run_density(dev, s, model, kw, selection=torch.from_numpy(kw["selection"].astype(np.uint8)).to(dev))
    assert torch.equal(u8.occ, f.occ)


def test_bounds_of_an_earlier_field_are_shared(dev):
    s, model, kw, truth, _ = case("random16")
    first = run_density(dev, s, model, kw)
    again = run_density(dev, s, model, kw, bounds=(first.center, first.scale))
    assert torch.equal(first.occ, again.occ) and torch.equal(first.center, again.center) and torch.equal(first.scale, again.scale)


def test_nothing_kept_and_an_empty_model(dev):
    from goi_hyperplane_amd import field
    s, model, kw, _truth, _ = case("batch16")
    f = run_density(dev, s, model, kw, min_opacity=2.0)
    assert float(f.occ.abs().max()) == 0 and float(f.attr.abs().max()) == 0
    assert f.center.tolist() == [0, 0, 0] and float(f.scale) == 1 and int(f.status) == 0
    z = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    e = field.density_grid(z(0, 3), z(0), z(0, 3), z(0, 4), 16, 2, attributes=z(0, 3))
    assert float(e.occ.abs().max()) == 0 and float(e.attr.abs().max()) == 0 and float(e.scale) == 1
    one = {k: v[40:41] for k, v in model.items()}  # a single kept Gaussian: no extent, scale 1, centred on it
    f = run_density(dev, s, one, {})
    assert np.array_equal(f.center.cpu().numpy(), one["xyz"][0]) and float(f.scale) == 1 and float(f.occ.max()) > 0


def test_density_grid_never_synchronises(dev):
    s, model, kw, _truth, _ = case("clusters24_sel")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    from goi_hyperplane_amd import field
    args = [t(model[k]) for k in ("xyz", "opacity", "scaling", "rotation")]
    sel, rgb = t(kw["selection"]), t(model["rgb"])
    first = field.density_grid(*args, 24, 6, 0.25)  # loads the library and warms up outside the checked region
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        f = field.density_grid(*args, 24, 6, 0.25, selection=sel, selection_invert=True, attributes=rgb,
                               bounds=(first.center, first.scale))
        g = field.density_grid(*args, 24, 6, 0.25)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(g.occ, first.occ) and f.attr is not None


# ---- iso-surface ------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_iso(dev, grid, thresh, attr=None, coords=None):
    from goi_hyperplane_amd import field
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dc = None if coords is None else (tuple(t(c) for c in coords) if isinstance(coords, tuple) else t(coords))
    out = field.isosurface(t(grid), thresh, None if attr is None else t(attr), dc)
    v, f, c = ref.marching_tets(grid, thresh, attr, coords)
    assert out.faces.dtype == torch.int32 and tuple(out.faces.shape) == f.shape and tuple(out.vertices.shape) == v.shape
    assert np.array_equal(out.faces.cpu().numpy(), f)
    assert np.array_equal(bits(out.vertices.cpu().numpy()), bits(v))
    if attr is None:
        assert out.colors is None
    else:
        assert np.array_equal(bits(out.colors.cpu().numpy()), bits(c))
    return out


def test_isosurface_on_the_analytic_grids(dev):
    for make in (ref.sphere_grid, ref.torus_grid, ref.two_spheres_grid, ref.plane_grid, ref.equal_grid):
        g, th = make()
        check_iso(dev, g, th)
    g, th = ref.sphere_grid()
    check_iso(dev, g, th, ref.grid_attributes(g.shape), np.linspace(-1, 1, 16).astype(np.float32))
    g, th = ref.torus_grid()  # [24, 24, 12]: one table per axis
    axes = tuple(np.sort(np.random.default_rng(i).uniform(-2, 3, size=n)).astype(np.float32) for i, n in enumerate(g.shape))
    out = check_iso(dev, g, th, ref.grid_attributes(g.shape), axes)
    top = ref.mesh_topology(out.faces.cpu().numpy(), out.vertices.shape[0])
    assert top["chi"] == 0 and set(top["edge_use"]) == {2}
    g, th = ref.two_spheres_grid()  # [24, 14, 13], index coordinates, colours
    check_iso(dev, g, th, ref.grid_attributes(g.shape))


def test_isosurface_empty_results_and_thin_grids(dev):
    for value in (0.0, 5.0):
        out = check_iso(dev, np.full((6, 7, 5), value, np.float32), 1.0, np.ones((3, 6, 7, 5), np.float32))
        assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.colors.shape) == (0, 3)
    g = np.random.default_rng(3).uniform(0, 2, size=(9, 1, 6)).astype(np.float32)  # no cube: vertices without faces
    out = check_iso(dev, g, 1.0)
    assert out.faces.shape[0] == 0 and out.vertices.shape[0] > 0
    check_iso(dev, np.random.default_rng(4).uniform(0, 2, size=(1, 1, 1)).astype(np.float32), 1.0)
    g = np.random.default_rng(5).uniform(0, 2, size=(5, 4, 3)).astype(np.float32)
    g[1, 2, 1] = np.nan  # a NaN is outside
    from goi_hyperplane_amd import field
    out = field.isosurface(torch.from_numpy(g).to(dev), 1.0)
    assert np.array_equal(out.faces.cpu().numpy(), ref.marching_tets(g, 1.0)[1])


def test_isosurface_across_scan_chunks(dev):
    g, th = ref.noisy_grid()  # 40^3: 128000 counts, 215 k vertices, 445 k faces
    out = check_iso(dev, g, th, ref.grid_attributes(g.shape))
    assert out.vertices.shape[0] > 200000 and out.faces.shape[0] > 400000
    again = check_iso(dev, g, th)
    assert torch.equal(out.faces, again.faces) and torch.equal(out.vertices, again.vertices)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def gaussian_set(dev, m, keep=None):
    from goi_hyperplane_amd.render import GaussianSet
    idx = slice(None) if keep is None else keep
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[idx])).to(dev)  # noqa: E731
    P = len(m["opacity"][idx])
    shs = torch.zeros((P, 16, 3), device=dev)
    shs[:, 0, :] = (t(m["rgb"]) - 0.5) / ref.SH_C0
    return GaussianSet(t(m["xyz"]), t(m["scaling"]), t(m["rotation"]), t(m["opacity"]).reshape(-1, 1), shs,
                       torch.zeros((P, 10), device=dev))


@pytest.fixture(scope="module")
def shell(dev):
    from goi_hyperplane_amd import field
    m = ref.sphere_shell_model(2000)
    pc = gaussian_set(dev, m)
    return m, pc, field.extract_mesh(pc, m["thresh"], resolution=32, num_blocks=2)


def test_extract_mesh_on_a_shell(dev, shell):
    from goi_hyperplane_amd import field
    m, pc, mesh = shell
    f = field.density_grid(pc.get_xyz, pc.get_opacity, pc.get_scaling, pc.get_rotation, 32, 2, attributes=torch.from_numpy(m["rgb"]).to(dev))
    coords = f.coords.cpu().numpy()
    v, faces, c = ref.marching_tets(f.occ.cpu().numpy(), m["thresh"], f.attr.cpu().numpy(), coords)
    assert np.array_equal(mesh.faces.cpu().numpy(), faces) and len(faces) > 5000
    top = ref.mesh_topology(faces, len(v))
    assert set(top["edge_use"]) == {2} and top["consistent"] and top["all_used"] and top["chi"] == 2
    scale, center = float(mesh.scale), mesh.center.cpu().numpy()
    assert np.array_equal(center, f.center.cpu().numpy()) and scale == float(f.scale)
    world = mesh.vertices.cpu().numpy().astype(np.float64)
    assert np.allclose(world, v.astype(np.float64) / scale + center, rtol=0, atol=1e-5)
    spacing = (coords[1] - coords[0]) / scale
    d = np.linalg.norm(world - m["shell_center"], axis=1)
    print(f"\nshell: {len(v)} vertices, {len(faces)} faces, |distance - radius| <= {np.abs(d - m['shell_radius']).max():.4f}, "
          f"grid spacing {spacing:.4f}")
    assert np.all(np.abs(d - m["shell_radius"]) < spacing)
    n, cen = ref.face_normals(world, faces)
    assert np.all(np.einsum("ij,ij->i", n, cen - m["shell_center"]) > 0)
    # "rgb" = 0.5 + C0 f_dc: the colours of the explicit tensor up to the rounding of that round trip, inside [0, 1]
    col = mesh.colors.cpu().numpy()
    assert col.min() >= 0 and col.max() <= 1 and np.abs(col - np.clip(c, 0, 1)).max() < 1e-5
    assert 0.3 < col.mean() < 0.7  # the average of uniform colours, not 0 or 1


def test_extract_mesh_colour_modes(dev, shell):
    from goi_hyperplane_amd import field
    m, pc, mesh = shell
    plain = field.extract_mesh(pc, m["thresh"], resolution=32, num_blocks=2, colors=None)
    assert plain.colors is None and torch.equal(plain.faces, mesh.faces) and torch.equal(plain.vertices, mesh.vertices)
    rgb = torch.from_numpy(m["rgb"]).to(dev)
    given = field.extract_mesh(pc, m["thresh"], resolution=32, num_blocks=2, colors=rgb)
    f = field.density_grid(pc.get_xyz, pc.get_opacity, pc.get_scaling, pc.get_rotation, 32, 2, attributes=rgb)
    c = ref.marching_tets(f.occ.cpu().numpy(), m["thresh"], f.attr.cpu().numpy(), f.coords.cpu().numpy())[2]
    assert np.array_equal(bits(given.colors.cpu().numpy()), bits(np.clip(c, 0, 1)))
    assert torch.equal(given.faces, mesh.faces)


def test_extract_mesh_refuses_a_grid_whose_sort_failed(dev, shell, monkeypatch):
    from goi_hyperplane_amd import field
    m, pc, _mesh = shell
    real = field.density_grid

    def failed(*a, **k):
        f = real(*a, **k)
        return f._replace(status=torch.full_like(f.status, 2))
    monkeypatch.setattr(field, "density_grid", failed)
    with pytest.raises(RuntimeError, match="status 2"):
        field.extract_mesh(pc, m["thresh"], resolution=32, num_blocks=2)


def test_extract_mesh_of_a_selection(dev, shell, tmp_path):
    """Every second Gaussian: half the density everywhere, so half the threshold gives the same shell."""
    from goi_hyperplane_amd import field
    from goi_hyperplane_amd import io as gio
    m, pc, mesh = shell
    keep = np.arange(2000) % 2 == 0
    sel = torch.from_numpy(keep).to(dev)
    frame = (mesh.center, mesh.scale)
    a = field.extract_mesh(pc, m["thresh"] / 2, resolution=32, num_blocks=2, selection=sel, bounds=frame)
    b = field.extract_mesh(gaussian_set(dev, m, keep), m["thresh"] / 2, resolution=32, num_blocks=2, bounds=frame)
    assert a.faces.shape[0] > 5000
    assert torch.equal(a.faces, b.faces) and torch.equal(a.vertices, b.vertices) and torch.equal(a.colors, b.colors)
    inv = field.extract_mesh(pc, m["thresh"] / 2, resolution=32, num_blocks=2, selection=~sel, selection_invert=True, bounds=frame)
    assert torch.equal(inv.faces, a.faces) and torch.equal(inv.vertices, a.vertices)
    top = ref.mesh_topology(a.faces.cpu().numpy(), a.vertices.shape[0])
    assert top["chi"] == 2 and set(top["edge_use"]) == {2}
    p = str(tmp_path / "half.ply")
    gio.save_mesh_ply(p, a.vertices, a.faces, a.colors)
    v, f, c = gio.read_mesh_ply(p)
    assert np.array_equal(v, a.vertices.cpu().numpy()) and np.array_equal(f, a.faces.cpu().numpy()) and c.shape == v.shape
