"""The mesh stage without a GPU: the restatements of tests/field_reference.py against the reference's own
gaussian_3d_coeff / build_scaling_rotation / strip_symmetric (tests/golden/ref_field_pins.npz, made by
tests/golden/make_field_golden.py), the marching-tetrahedra restatement on analytic grids (closed, oriented, the right
Euler characteristic), the mesh PLY round trip, the C ABI's declarations, and the argument checks of
goi_hyperplane_amd.field that run on the host before anything is launched."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

from tests import field_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "golden", "ref_field_pins.npz")
HEADER = os.path.join(HERE, "..", "include", "goi_raster.h")


@pytest.fixture(scope="module")
def pins():
    with np.load(PINS) as z:
        return {k: z[k] for k in z.files}


# ---- the pins ---------------------------------------------------------------------------------------------------------------
def test_the_pins_hold_the_hard_rows(pins):
    w = pins["coeff_w"]
    assert w.shape == (400,) and pins["sr_L"].shape == (320, 3, 3)
    assert (w == 0).sum() >= 20 and ((w > 0) & (w < 1)).sum() >= 200 and np.isfinite(w).all()
    cov = pins["coeff_cov"].astype(np.float64)
    a, b, c, d, e, f = cov.T
    det = a * d * f + 2 * e * c * b - e**2 * a - c**2 * d - b**2 * f
    assert (det == 0).sum() >= 30  # the 1e-24 decides
    assert (np.abs(det) < 1e-6 * np.abs(a * d * f) + 1e-30).sum() >= 60  # those and the near-singular rows (float32 noise of a
    # determinant that is 1e-8 of its terms)
    assert (det < 0).sum() >= 30  # indefinite rows


def test_float32_restatements_reproduce_the_reference_bit_for_bit(pins):
    t = torch.from_numpy
    w = ref.pair_weight(t(pins["coeff_xyz"]), t(pins["coeff_cov"])).numpy()
    assert np.array_equal(w, pins["coeff_w"])
    L = ref.scaled_rotation(t(pins["sr_scale"]), t(pins["sr_rot"]))
    assert np.array_equal(L.numpy(), pins["sr_L"])
    assert np.array_equal(ref.packed_symmetric(L @ L.transpose(1, 2)).numpy(), pins["sr_cov"])
    assert np.array_equal(ref.covariance6(t(pins["sr_scale"]), t(pins["sr_rot"])).numpy(), pins["sr_cov"])


def test_numpy_coefficient_restatement_reproduces_the_reference(pins):
    """float32 numpy: numpy's exp and torch's may differ in the last bit; float64: within float32 rounding of the pins where
    the row is well conditioned (the reference's own error grows with the cancellation in its determinant)."""
    with np.errstate(all="ignore"):
        w32 = ref.pair_weight(pins["coeff_xyz"], pins["coeff_cov"])
    assert w32.dtype == np.float32
    assert np.all(np.abs(w32 - pins["coeff_w"]) <= 2 * ref.EPS32 * pins["coeff_w"] + 1e-44)
    assert np.array_equal(w32 == 0, pins["coeff_w"] == 0)
    cov = pins["coeff_cov"].astype(np.float64)
    with np.errstate(all="ignore"):
        w64 = ref.pair_weight(pins["coeff_xyz"].astype(np.float64), cov)
    a, b, c, d, e, f = cov.T
    det = a * d * f + 2 * e * c * b - e**2 * a - c**2 * d - b**2 * f
    good = (det > 1e-3 * a * d * f) & (w64 > 1e-8)  # (a weight of 1e-30 carries the float32 rounding of a power of -69)
    assert good.sum() >= 150
    assert np.all(np.abs(w64[good] - pins["coeff_w"][good]) <= 1e-3 * w64[good] + 1e-30)


def test_float64_covariance_reproduces_the_reference(pins):
    c64 = ref.covariance6(pins["sr_scale"].astype(np.float64), pins["sr_rot"].astype(np.float64))
    scale = np.abs(c64).max(axis=1, keepdims=True)
    assert np.all(np.abs(c64 - pins["sr_cov"]) <= 16 * ref.EPS32 * scale)


# ---- marching tetrahedra ----------------------------------------------------------------------------------------------------
def test_case_table_is_complete_and_consistent():
    table = ref.case_table()
    assert len(table) == 6 and all(len(row) == 16 for row in table)
    for row in table:
        assert row[0] == [] and row[15] == []
        for m in range(1, 15):
            assert len(row[m]) == (2 if bin(m).count("1") == 2 else 1)
            # the complementary case crosses the same edges with the opposite orientation
            flip = [(t[0], t[2], t[1]) for t in row[15 - m]]
            assert sorted(map(sorted, row[m])) == sorted(map(sorted, flip))


def closed(top):
    return set(top["edge_use"]) == {2} and top["consistent"] and top["all_used"]


def test_sphere_is_closed_oriented_and_genus_zero():
    for shape, c, r in (((16, 16, 16), (7.3, 7.6, 7.1), 5.2), ((12, 14, 13), (5.4, 6.3, 6.2), 4.1), ((24, 24, 24), (11.2, 12.1, 11.7), 9.3)):
        g, th = ref.sphere_grid(shape, c, r)
        v, f, _ = ref.marching_tets(g, th)
        top = ref.mesh_topology(f, len(v))
        assert closed(top) and top["chi"] == 2, (shape, top)
        n, cen = ref.face_normals(v, f)
        assert np.all(np.einsum("ij,ij->i", n, cen - np.array(c)) > 0), "a normal points inwards"
        assert np.all(np.abs(np.linalg.norm(v - np.array(c), axis=1) - r) < 0.35)  # linear interpolation of a distance field
        assert f.min() >= 0 and f.max() < len(v) and f.dtype == np.int32


def test_torus_and_two_spheres():
    g, th = ref.torus_grid()
    v, f, _ = ref.marching_tets(g, th)
    top = ref.mesh_topology(f, len(v))
    assert closed(top) and top["chi"] == 0, top
    g, th = ref.two_spheres_grid()
    v, f, _ = ref.marching_tets(g, th)
    top = ref.mesh_topology(f, len(v))
    assert closed(top) and top["chi"] == 4, top


def test_plane_is_open_only_at_the_grid_boundary():
    g, th = ref.plane_grid()
    v, f, _ = ref.marching_tets(g, th)
    top = ref.mesh_topology(f, len(v))
    assert set(top["edge_use"]) == {1, 2} and top["consistent"] and top["chi"] == 1, top
    hi = np.array(g.shape) - 1
    for a, b in top["boundary_edges"]:
        on = lambda p: np.isclose(p, 0) | np.isclose(p, hi)  # noqa: E731
        assert np.any(on(v[a]) & on(v[b])), "a boundary edge inside the grid"
    n, _ = ref.face_normals(v, f)
    assert np.all(n @ np.array((0.3137, 0.5219, 0.8043)) > 0)  # inside is below the plane: normals point up it


def test_uniform_grids_give_an_empty_mesh():
    for value in (0.0, 5.0):
        v, f, c = ref.marching_tets(np.full((6, 7, 5), value, np.float32), 1.0, attr=np.zeros((3, 6, 7, 5), np.float32))
        assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)


def test_points_equal_to_the_threshold_are_outside():
    g, th = ref.equal_grid()
    assert (g == th).sum() > 90
    v, f, _ = ref.marching_tets(g, th)
    top = ref.mesh_topology(f, len(v))
    assert closed(top) and top["chi"] == 2
    assert f.min() >= 0 and f.max() < len(v)
    # every vertex sits ON a threshold point (t = 1 from the inside owner, or 0 from an outside one): the surface is the shell
    # of threshold points, and faces collapse to zero area where several crossings meet in one point -- their indices stay valid
    assert np.all(np.abs(np.abs(v - 5.0).max(axis=1) - 2.0) < 1e-6)


def test_float64_and_float32_surfaces_agree():
    g, th = ref.sphere_grid()
    a = ref.grid_attributes(g.shape)
    v32, f32, c32 = ref.marching_tets(g, th, a)
    v64, f64, c64 = ref.marching_tets(g, th, a, dtype=np.float64)
    assert np.array_equal(f32, f64) and v32.dtype == np.float32 and c32.dtype == np.float32
    assert np.abs(v32 - v64).max() < 1e-4 and np.abs(c32 - c64).max() < 1e-4


# ---- PLY --------------------------------------------------------------------------------------------------------------------
def test_mesh_ply_round_trip(tmp_path):
    from goi_hyperplane_amd import io as gio
    g, th = ref.sphere_grid()
    v, f, c = ref.marching_tets(g, th, ref.grid_attributes(g.shape))
    c = np.clip(c, 0, 1)
    p = str(tmp_path / "sub" / "mesh.ply")
    gio.save_mesh_ply(p, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(c))
    head = open(p, "rb").read(400).split(b"end_header\n")[0].decode()
    assert head.splitlines()[:2] == ["ply", "format binary_little_endian 1.0"]
    assert "property uchar red" in head and "property list uchar int vertex_indices" in head
    v2, f2, c2 = gio.read_mesh_ply(p)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and f2.dtype == np.int32
    assert np.array_equal(c2, np.rint(c * 255).astype(np.uint8))
    assert os.path.getsize(p) == len(head) + len("end_header\n") + len(v) * 15 + len(f) * 13
    gio.save_mesh_ply(p, v, f)
    v2, f2, c2 = gio.read_mesh_ply(p)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and c2 is None
    for colors in (None, np.zeros((0, 3), np.float32)):
        gio.save_mesh_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), colors)
        v2, f2, c2 = gio.read_mesh_ply(p)
        assert v2.shape == (0, 3) and f2.shape == (0, 3) and (c2 is None) == (colors is None)
    gio.save_mesh_ply(p, v, np.zeros((0, 3), np.int32))
    assert gio.read_mesh_ply(p)[1].shape == (0, 3)
    with pytest.raises(ValueError):
        gio.save_mesh_ply(p, v, f + len(v))


# ---- the ABI and the argument checks ------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_agree():
    from goi_hyperplane_amd import _lib, build, field
    build.build()
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(goi_field_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.FIELD_SYMBOLS) and len(declared) == 5
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
    define = lambda n: re.search(rf"#define {n} ([0-9.]+)", hdr).group(1)  # noqa: E731
    assert int(define("GOI_FIELD_BATCH")) == field.BATCH
    assert (int(define("GOI_FIELD_MIN_SPLIT")), int(define("GOI_FIELD_MAX_SPLIT"))) == (field.MIN_SPLIT, field.MAX_SPLIT)
    assert int(define("GOI_FIELD_MAX_RESOLUTION")) == field.MAX_RESOLUTION and float(define("GOI_FIELD_MAX_RELAX")) == field.MAX_RELAX
    # the size queries refuse what the entry points refuse
    assert lib.goi_field_density_workspace_bytes(1000, 128, 16, 1.5) > 0
    for bad in ((1000, 128, 15, 1.5), (1000, 128, 64, 1.5), (1000, 128, 4, 1.5), (1000, 512, 32, 1.5), (1000, 128, 16, 4.5),
                (0, 128, 16, 1.5), (2 ** 30, 128, 16, 1.5)):
        assert lib.goi_field_density_workspace_bytes(*bad) == 0, bad
    assert lib.goi_field_iso_workspace_bytes(40, 40, 40) > 0
    assert lib.goi_field_iso_workspace_bytes(0, 4, 4) == 0 and lib.goi_field_iso_workspace_bytes(1024, 1024, 1024) == 0
    assert lib.goi_field_iso_workspace_bytes(512, 512, 256) > 0 and lib.goi_field_iso_workspace_bytes(512, 512, 257) == 0  # 2^26
    # and the entries themselves, before they touch a pointer
    assert lib.goi_field_density(10, *[None] * 5, 0, 0.005, None, None, 128, 15, 1.5, *[None] * 9) < 0
    assert "num_blocks" in _lib.last_error()
    assert lib.goi_field_iso_count(None, 0, 4, 4, 1.0, None, None, None) < 0


def model(P=10):
    g = torch.Generator().manual_seed(0)
    return dict(xyz=torch.randn(P, 3, generator=g), opacity=torch.rand(P, generator=g), scaling=torch.rand(P, 3, generator=g) + 0.1,
                rotation=torch.randn(P, 4, generator=g))


def test_density_grid_argument_checks():
    from goi_hyperplane_amd import field
    m = model()
    for kw in (dict(resolution=100, num_blocks=16), dict(resolution=128, num_blocks=64), dict(resolution=128, num_blocks=4),
               dict(resolution=512, num_blocks=32), dict(relax_ratio=4.5), dict(relax_ratio=-1.0), dict(num_blocks=0),
               dict(min_opacity=float("nan")), dict(bounds=(torch.zeros(3),))):
        with pytest.raises(ValueError):
            field.density_grid(**m, **kw)
    for key, bad in (("xyz", torch.zeros(10, 2)), ("xyz", m["xyz"].double()), ("opacity", torch.zeros(9)),
                     ("scaling", torch.zeros(10, 4)), ("rotation", torch.zeros(10, 3)), ("rotation", m["rotation"].half())):
        with pytest.raises(ValueError):
            field.density_grid(**{**m, key: bad})
    with pytest.raises(ValueError):
        field.density_grid(**m, selection=torch.zeros(9, dtype=torch.bool))
    with pytest.raises(ValueError):
        field.density_grid(**m, selection=torch.zeros(10))
    with pytest.raises(ValueError):
        field.density_grid(**m, attributes=torch.zeros(10, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        field.density_grid(**m)
    assert field.check_grid(128, 16, 1.5) == 8 and field.check_grid(256, 16, 4.0) == 16 and field.check_grid(24, 6, 0.0) == 4


def test_isosurface_and_extract_mesh_argument_checks():
    from goi_hyperplane_amd import field
    g = torch.zeros(4, 5, 6)
    for bad in (torch.zeros(4, 5), g.double(), torch.zeros(0, 5, 6), torch.zeros(1, 1, 1).expand(512, 512, 257)):
        with pytest.raises(ValueError):
            field.isosurface(bad, 1.0)
    with pytest.raises(ValueError):
        field.isosurface(g, float("nan"))
    with pytest.raises(ValueError):
        field.isosurface(g, 1.0, attributes=torch.zeros(3, 4, 5, 5))
    with pytest.raises(ValueError):
        field.isosurface(g, 1.0, coords=torch.zeros(4))  # one table serves a cubic grid only
    with pytest.raises(ValueError):
        field.isosurface(g, 1.0, coords=(torch.zeros(4), torch.zeros(5)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        field.isosurface(g, 1.0)

    class PC:
        get_xyz, get_opacity, get_scaling, get_rotation = (model()[k] for k in ("xyz", "opacity", "scaling", "rotation"))
        get_features = torch.zeros(10, 16, 3)
    with pytest.raises(ValueError):
        field.extract_mesh(PC(), colors="semantic")
    with pytest.raises(ValueError):
        field.extract_mesh(PC(), colors=torch.zeros(10, 4))
    with pytest.raises(ValueError):
        field.extract_mesh(PC(), resolution=100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        field.extract_mesh(PC())
