"""A mesh from the Gaussians on the device (csrc/field.hip): the density grid and its iso-surface.  The reference's three
viewers call `self.renderer.gaussians.extract_mesh(path, self.opt.density_thresh)` (gui/main.py:607-617,
gui/main_edit.py:821-836, gui/main_test.py:849-858) on a GaussianModel that has no such method: only gaussian_3d_coeff
(gui/gs_renderer.py:66-85) survived its port from DreamGaussian.  This module is that method.

    density_grid   DreamGaussian's extract_fields(resolution=128, num_blocks=16, relax_ratio=1.5): occ[x, y, z] =
                   sum opacity_i w_i over the Gaussians of the point's block, optionally sum opacity_i w_i a_i as well
    isosurface     marching tetrahedra (Kuhn split) of any [X, Y, Z] grid: watertight by construction, deterministic order
    extract_mesh   both, with the vertices mapped back to world coordinates

Semantics of density_grid (tests/field_reference.py restates them in float64):
  * kept: activated opacity > min_opacity (strictly, compared in float32), selected (`selection` is honoured in place: the
    model is not index-selected), finite centre;
  * frame: center = (amin + amax) / 2 of the kept centres, scale = 1.8 / max extent, computed on the device; `bounds` =
    (center, scale) of an earlier DensityField lets a whole edit session share one frame.  Nothing kept: center 0, scale 1;
    kept centres without extent: scale 1;
  * centres and activated scales are multiplied by scale; covariance (R S)(R S)^T of the normalised quaternion, as
    build_scaling_rotation / strip_symmetric; weight as gaussian_3d_coeff writes it (inverse through
    1 / (det + 1e-24), formed once per Gaussian in float64 and rounded; power > 0 gives 0);
  * the grid is torch.linspace(-1, 1, R) per axis, handed to the kernel as a table; a Gaussian joins a block iff its
    centre lies strictly inside the block's point bounds widened by (2 / num_blocks) * relax_ratio (float32), as the
    reference's mask does.  Membership goes by centre, not by extent.

Everything runs on the current stream.  density_grid reads nothing back; isosurface reads its two counts back once to size
its outputs.  No float atomics: results are bit-identical from run to run.  There is no CPU fallback.

Not here: the reference's follow-ups clean_mesh / decimate_mesh and the normals of Mesh.auto_normal (mesh.py has them:
mesh.extract chains them behind extract_mesh), UV unwrapping and the nvdiffrast texture bake of mode='geo+tex'.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from ._lib import check, ptr, stream, workspace

# GOI_FIELD_* of include/goi_raster.h
BATCH = 128  # members a block stages in LDS before its threads consume them
MIN_SPLIT, MAX_SPLIT, MAX_RESOLUTION, MAX_RELAX = 4, 16, 256, 4.0
MAX_GRID_POINTS = 2 ** 26
SH_C0 = 0.28209479177387814
_NO_CPU = "goi_hyperplane_amd.field: tensors must live on a ROCm GPU; there is no CPU fallback"

DensityField = namedtuple("DensityField", "occ attr center scale coords status")
DensityField.__doc__ = """occ float32 [R, R, R] indexed [x, y, z]; attr float32 [3, R, R, R] or None; center [3] and scale (0-d) device
tensors: normalised = (world - center) * scale; coords float32 [R]; status int32 0-d device tensor: 0, or non-zero when the
sort's look-back timed out on a wedged device and the grids are garbage.  density_grid reads nothing back, so it cannot
raise for it: check `status` where you read the grids back (extract_mesh does, and raises)."""
IsoSurface = namedtuple("IsoSurface", "vertices faces colors")
Mesh = namedtuple("Mesh", "vertices faces colors center scale")


def check_grid(resolution, num_blocks, relax_ratio) -> int:
    """split = resolution // num_blocks of a supported grid; ValueError otherwise."""
    R, nb = int(resolution), int(num_blocks)
    if R != resolution or nb != num_blocks or nb < 1 or R < 1:
        raise ValueError(f"field: resolution and num_blocks must be positive integers, got {resolution!r}, {num_blocks!r}")
    if R > MAX_RESOLUTION:
        raise ValueError(f"field: resolution must be <= {MAX_RESOLUTION}, got {R}")
    if R % nb != 0:
        raise ValueError(f"field: resolution {R} is not a multiple of num_blocks {nb}")
    split = R // nb
    if not MIN_SPLIT <= split <= MAX_SPLIT:
        raise ValueError(f"field: resolution / num_blocks must be in {MIN_SPLIT} .. {MAX_SPLIT}, got {split}")
    rr = float(relax_ratio)
    if not 0.0 <= rr <= MAX_RELAX:
        raise ValueError(f"field: relax_ratio must be in 0 .. {MAX_RELAX}, got {relax_ratio!r}")
    return split


def _f32(fn, name, t, shape):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{fn}: {name} must be float32, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{fn}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _selection(fn, sel, P):
    if sel is None:
        return None
    if not isinstance(sel, torch.Tensor) or sel.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{fn}: selection must be a bool or uint8 tensor")
    if tuple(sel.shape) != (P,):
        raise ValueError(f"{fn}: selection must have shape ({P},), got {tuple(sel.shape)}")
    return sel


def block_bounds(coords: torch.Tensor, num_blocks: int, relax_ratio: float):
    """The widened point bounds of every block along one axis, (lo [num_blocks], hi [num_blocks]), formed as the reference
    forms them: amin / amax of the block's points, -= / += block_size * relax_ratio in float32."""
    split = int(coords.numel()) // int(num_blocks)
    w = (2 / num_blocks) * relax_ratio
    return (coords[0::split] - w).contiguous(), (coords[split - 1::split] + w).contiguous()


def density_grid(xyz, opacity, scaling, rotation, resolution=128, num_blocks=16, relax_ratio=1.5, min_opacity=0.005,
                 selection=None, selection_invert=False, attributes=None, bounds=None) -> DensityField:
    """xyz [P, 3], opacity [P] or [P, 1] (activated), scaling [P, 3] (activated), rotation [P, 4] (any norm), all float32.
    selection: bool / uint8 [P]; attributes: float32 [P, 3]; bounds: (center [3], scale) as tensors or numbers.
    See the module docstring for the semantics.  split = resolution // num_blocks must be in 4 .. 16, resolution <= 256,
    relax_ratio <= 4.  Nothing is read back: look at the result's `status` before trusting grids you copy to the host."""
    fn = "field.density_grid"
    check_grid(resolution, num_blocks, relax_ratio)
    R, nb = int(resolution), int(num_blocks)
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{fn}: xyz must be a [P, 3] tensor")
    P = int(xyz.shape[0])
    if P >= 2 ** 30:
        raise ValueError(f"{fn}: need P < 2^30, got {P}")
    _f32(fn, "xyz", xyz, (P, 3))
    if isinstance(opacity, torch.Tensor) and tuple(opacity.shape) == (P, 1):
        opacity = opacity.reshape(P)
    _f32(fn, "opacity", opacity, (P,))
    _f32(fn, "scaling", scaling, (P, 3))
    _f32(fn, "rotation", rotation, (P, 4))
    if attributes is not None:
        _f32(fn, "attributes", attributes, (P, 3))
    _selection(fn, selection, P)
    mo = float(min_opacity)
    if mo != mo:
        raise ValueError(f"{fn}: min_opacity is NaN")
    if bounds is not None and (not isinstance(bounds, (tuple, list)) or len(bounds) != 2):
        raise ValueError(f"{fn}: bounds must be (center, scale)")
    used = [xyz, opacity, scaling, rotation] + [t for t in (attributes, selection) if t is not None]
    if not all(t.is_cuda for t in used):
        raise RuntimeError(_NO_CPU)
    dev = xyz.device
    if any(t.device != dev for t in used):
        raise ValueError(f"{fn}: all tensors must live on one device")

    frame_in = None
    if bounds is not None:
        c = torch.as_tensor(bounds[0], dtype=torch.float32, device=dev).reshape(-1)
        s = torch.as_tensor(bounds[1], dtype=torch.float32, device=dev).reshape(-1)
        if c.numel() != 3 or s.numel() != 1:
            raise ValueError(f"{fn}: bounds must be (center [3], scale)")
        frame_in = torch.cat([c, s])
    lib = _lib.load()
    coords = torch.linspace(-1, 1, R, dtype=torch.float32, device=dev)
    lo, hi = block_bounds(coords, nb, float(relax_ratio))
    occ = torch.empty((R, R, R), dtype=torch.float32, device=dev)
    attr = torch.empty((3, R, R, R), dtype=torch.float32, device=dev) if attributes is not None else None
    frame = torch.empty(4, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    sel = None
    if selection is not None:
        sel = selection.contiguous()
        sel = sel.view(torch.uint8) if sel.dtype == torch.bool else sel
    src = [t.detach().contiguous() for t in (xyz, opacity, scaling, rotation)]
    att = attributes.detach().contiguous() if attributes is not None else None
    ws = None
    if P > 0:
        ws = workspace(lib.goi_field_density_workspace_bytes(P, R, nb, float(relax_ratio)), dev)
    with torch.cuda.device(dev):
        check(lib.goi_field_density(P, ptr(src[0]), ptr(src[1]), ptr(src[2]), ptr(src[3]), ptr(sel), 1 if selection_invert else 0,
                                    mo, ptr(att), ptr(frame_in), R, nb, float(relax_ratio), ptr(coords), ptr(lo), ptr(hi),
                                    ptr(occ), ptr(attr), ptr(frame), ptr(status), ptr(ws), stream(dev)))
    return DensityField(occ, attr, frame[:3], frame[3], coords, status[0])


def _axis_tables(fn, coords, shape):
    if coords is None:
        return [None, None, None]
    if isinstance(coords, torch.Tensor):
        coords = (coords, coords, coords)
    if not isinstance(coords, (tuple, list)) or len(coords) != 3:
        raise ValueError(f"{fn}: coords must be one [n] tensor (a cubic grid) or three, one per axis")
    return [_f32(fn, f"coords[{axis}]", t, (n,)) for axis, (t, n) in enumerate(zip(coords, shape))]


def isosurface(grid, thresh, attributes=None, coords=None) -> IsoSurface:
    """The surface value == thresh of a float32 [X, Y, Z] grid by marching tetrahedra on the Kuhn split of every cube.  A
    point is inside iff value > thresh.  attributes: float32 [3, X, Y, Z] sums (DensityField.attr); the colour of a vertex
    is their interpolation divided by thresh, the interpolated density at the crossing.  coords: the grid lines' coordinates
    (one [n] tensor for a cubic grid, or one per axis); default: the indices.
    -> vertices float32 [V, 3] ordered by (owner point, edge slot), faces int32 [F, 3] ordered by (cube, tetrahedron,
    triangle) with normals from inside to outside, colors float32 [V, 3] or None.  The surface is open where it meets the
    grid's boundary; V = F = 0 for a grid entirely inside or outside.  Reads the two counts back once."""
    fn = "field.isosurface"
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
        raise ValueError(f"{fn}: grid must be a [X, Y, Z] tensor")
    X, Y, Z = (int(n) for n in grid.shape)
    _f32(fn, "grid", grid, (X, Y, Z))
    if min(X, Y, Z) < 1 or X * Y * Z > MAX_GRID_POINTS:
        raise ValueError(f"{fn}: need X, Y, Z >= 1 and X * Y * Z <= 2^26, got {(X, Y, Z)}")
    t = float(thresh)
    if t != t:
        raise ValueError(f"{fn}: thresh is NaN")
    if attributes is not None:
        _f32(fn, "attributes", attributes, (3, X, Y, Z))
    tables = _axis_tables(fn, coords, (X, Y, Z))
    used = [grid] + [t for t in [attributes] + tables if t is not None]
    if not all(t.is_cuda for t in used):
        raise RuntimeError(_NO_CPU)
    dev = grid.device
    if any(t.device != dev for t in used):
        raise ValueError(f"{fn}: all tensors must live on one device")
    tables = [None if t is None else t.contiguous() for t in tables]

    lib = _lib.load()
    g = grid.detach().contiguous()
    a = attributes.detach().contiguous() if attributes is not None else None
    ws = workspace(lib.goi_field_iso_workspace_bytes(X, Y, Z), dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.goi_field_iso_count(ptr(g), X, Y, Z, t, ptr(ws), ptr(counts), stream(dev)))
        V, F = (int(n) for n in counts.tolist())  # the one read-back: the outputs' sizes
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        colors = torch.empty((V, 3), dtype=torch.float32, device=dev) if a is not None else None
        if V > 0 or F > 0:
            check(lib.goi_field_iso_emit(ptr(g), ptr(a), X, Y, Z, t, ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), ptr(ws),
                                         V, F, ptr(vertices), ptr(faces), ptr(colors), stream(dev)))
    return IsoSurface(vertices, faces, colors)


def _colors(fn, pc, colors, P):
    if colors is None:
        return None
    if isinstance(colors, str):
        if colors != "rgb":
            raise ValueError(f"{fn}: colors must be 'rgb', None or a [P, 3] tensor, got {colors!r}")
        return (0.5 + SH_C0 * pc.get_features.detach()[:, 0, :]).contiguous()
    return _f32(fn, "colors", colors, (P, 3))


def extract_mesh(pc, density_thresh=1.0, resolution=128, num_blocks=16, relax_ratio=1.5, selection=None,
                 selection_invert=False, colors="rgb", bounds=None, min_opacity=0.005) -> Mesh:
    """The iso-surface density == density_thresh of the model's density grid, in world coordinates: what the reference's
    "save mesh" button expects of GaussianModel.extract_mesh, without its pymeshlab clean-up and decimation.

    pc: anything with get_xyz / get_opacity / get_scaling / get_rotation (and get_features for "rgb").  density_thresh: the
    reference's configs ship no density_thresh; 1.0 is DreamGaussian's default.  selection / selection_invert: mesh only
    these Gaussians ("save what I selected"), in place.  colors: "rgb" (0.5 + C0 * f_dc), None, or a float32 [P, 3] tensor
    such as pca.gaussian_colors(pc).  bounds: (center, scale) of an earlier Mesh or DensityField, so that several
    extractions share one grid.  -> Mesh(vertices [V, 3] = v / scale + center, faces int32 [F, 3], colors [V, 3] clamped to
    [0, 1] or None, center, scale).  Save it with io.save_mesh_ply."""
    fn = "field.extract_mesh"
    xyz = pc.get_xyz.detach()
    att = _colors(fn, pc, colors, int(xyz.shape[0]))
    f = density_grid(xyz, pc.get_opacity.detach(), pc.get_scaling.detach(), pc.get_rotation.detach(), resolution, num_blocks,
                     relax_ratio, min_opacity, selection, selection_invert, att, bounds)
    iso = isosurface(f.occ, density_thresh, f.attr, f.coords)
    if int(f.status) != 0:  # (isosurface has read its counts back: the stream is drained, this costs one word)
        raise RuntimeError(f"{fn}: the density grid's sort timed out (status {int(f.status)}); the grid is not usable")
    vertices = iso.vertices / f.scale + f.center
    col = iso.colors.clamp(0.0, 1.0) if iso.colors is not None else None
    return Mesh(vertices, iso.faces, col, f.center, f.scale)
