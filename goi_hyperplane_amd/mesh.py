"""Mesh clean-up on the device (csrc/mesh.hip): what stands between field.extract_mesh's raw iso-surface and a
file a viewer can use.  The reference's "save mesh" path meant to run pymeshlab's clean_mesh / decimate_mesh
(gui/mesh_utils.py:44-147) and Mesh.auto_normal (gui/mesh.py:344-365) on the host; this module does that work on the GPU.

    components      connected components of the faces' vertex graph (CAS union-find; the label is the smallest vertex)
    clean           clean_mesh's filters: null faces, duplicate faces, small components (min_f faces / min_d % of the
                    diagonal), unreferenced vertices
    decimate        vertex clustering (the meshing_decimation_clustering alternative mesh_utils.py:65 names) on a
                    divisions^3 grid, the cluster mean as representative; `target_faces` bisects the divisions
    vertex_normals  Mesh.auto_normal: area-weighted face normals summed per vertex, in a fixed order
    extract         field.extract_mesh -> clean -> decimate -> vertex_normals

All functions take device tensors and run on the current stream.  Integer results are exact; no float is accumulated with
atomics, so results are bit-identical from run to run (tests/mesh_reference.py restates every function in numpy, and the
tests compare bits).  Counts are read back only to size outputs: components and vertex_normals read nothing back (look at
their `status` where you read the results back), clean reads back once, decimate once per probe of the bisection and once
more.  There is no CPU fallback.

The arithmetic of decimate, which is part of the contract: members are the finite vertices at least one face names; lo =
their per-axis minimum, e = their largest per-axis extent, cell = e / n, q = min(floor((v - lo) / cell), n - 1), all float32
and rounded once per operation (e == 0: every member in cell 0); a cell's representative is the float64 sum of its members
in ascending vertex index, divided by the count, rounded to float32; colours likewise, not clamped.

Vertex clustering does not preserve manifoldness: two sheets that pass through one cell are welded, and on the torus of the
tests at 16 divisions ten edges come out used three times.  Not here: quadric edge collapse (meshing_decimation_quadric_edge_
collapse, which is what decimate_mesh runs by default), isotropic remeshing, non-manifold repair (clean_mesh's
meshing_repair_non_manifold_*).  UV unwrapping and the texture bake of mode='geo+tex' are texture.py's:
texture.bake(pc, mesh.extract(pc, ...), bg_color) -> io.save_mesh_obj.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib, field
from ._lib import check, ptr, stream, workspace

# GOI_MESH_* of include/goi_raster.h
STATUS_SORT, STATUS_UNION, STATUS_RANGE = 2, 4, 8
MAX_DIVISIONS = 1024
MAX_KEYS = 2 ** 30
_NO_CPU = "goi_hyperplane_amd.mesh: tensors must live on a ROCm GPU; there is no CPU fallback"

Components = namedtuple("Components", "vertex_label face_label status")
Components.__doc__ = """vertex_label int32 [V]: the smallest vertex index of the vertex's component, -1 for a vertex no face names;
face_label int32 [F]: the label of the face's first vertex; status: int32 0-d device tensor of STATUS_* bits (0: fine).  Nothing was
read back, so nothing was raised: check_status(status) where you read the labels back."""
CleanMesh = namedtuple("CleanMesh", "vertices faces colors vertex_index face_index")
DecimatedMesh = namedtuple("DecimatedMesh", "vertices faces colors divisions cluster")
Mesh = namedtuple("Mesh", "vertices faces colors normals center scale")


def check_status(status, fn="mesh") -> None:
    """Raises for a non-zero status word (this reads it back)."""
    st = int(status)
    if st & STATUS_RANGE:
        raise ValueError(f"{fn}: a face names a vertex index outside 0 .. V - 1")
    if st:
        what = "a sort timed out" if st & STATUS_SORT else "the union-find ran out of its bound"
        raise RuntimeError(f"{fn}: {what} (status {st}); the result is not usable")


def _mesh_args(fn, vertices, faces, colors=None, n_vertices=None):
    """Validated (V, F, vertices, faces, colors, device); vertices may be None when n_vertices is given."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{fn}: faces must be a [F, 3] tensor")
    if faces.dtype != torch.int32:
        raise ValueError(f"{fn}: faces must be int32, got {faces.dtype}")
    F = int(faces.shape[0])
    if vertices is None:
        V = int(n_vertices)
        if V != n_vertices or V < 0:
            raise ValueError(f"{fn}: n_vertices must be a non-negative integer, got {n_vertices!r}")
    else:
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError(f"{fn}: vertices must be a [V, 3] tensor")
        V = int(vertices.shape[0])
        field._f32(fn, "vertices", vertices, (V, 3))
    if colors is not None:
        field._f32(fn, "colors", colors, (V, 3))
    if V >= MAX_KEYS or 3 * F >= MAX_KEYS:
        raise ValueError(f"{fn}: need V < 2^30 and 3 F < 2^30, got V = {V}, F = {F}")
    used = [t for t in (vertices, faces, colors) if t is not None]
    if not all(t.is_cuda for t in used):
        raise RuntimeError(_NO_CPU)
    dev = faces.device
    if any(t.device != dev for t in used):
        raise ValueError(f"{fn}: all tensors must live on one device")
    cont = [None if t is None else t.detach().contiguous() for t in (vertices, faces, colors)]
    return V, F, cont[0], cont[1], cont[2], dev


def components(faces, n_vertices) -> Components:
    """faces int32 [F, 3], n_vertices = V.  Two vertices are connected when a face names both.  Reads nothing back."""
    fn = "mesh.components"
    V, F, _, f, _, dev = _mesh_args(fn, None, faces, n_vertices=n_vertices)
    lib = _lib.load()
    vlabel = torch.empty(V, dtype=torch.int32, device=dev)
    flabel = torch.empty(F, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace(lib.goi_mesh_components_workspace_bytes(V, F), dev)
    with torch.cuda.device(dev):
        check(lib.goi_mesh_components(V, F, ptr(f), ptr(vlabel), ptr(flabel), ptr(status), ptr(ws), stream(dev)))
    return Components(vlabel, flabel, status[0])


def _empty(dev, colors, V):
    z = torch.empty
    return (z((0, 3), dtype=torch.float32, device=dev), z((0, 3), dtype=torch.int32, device=dev),
            None if colors is None else z((0, 3), dtype=torch.float32, device=dev))


def clean(vertices, faces, colors=None, min_faces=64, min_diag=0.2) -> CleanMesh:
    """clean_mesh's filters, in this order: (1) null faces -- a repeated index, a vertex with a non-finite coordinate, or a
    float32 cross product (v1 - v0) x (v2 - v0) that is exactly zero; (2) duplicate faces -- the same set of three indices in
    any rotation or orientation, the lowest face index stays; (3) components of what is left with fewer than min_faces faces,
    or with d2 < float64(min_diag)^2 * d2 of the mesh, d2 the float64 sum (x, y, z) of the squares of the float32 extents of
    the box, the mesh's box covering the vertices still referenced after (1) and (2); (4) unreferenced vertices.  The defaults
    are clean_mesh's min_f = 64 and min_d = 20 (%); min_faces = 0, min_diag = 0 keeps every component.
    -> CleanMesh: survivors in their order, faces renumbered in their cyclic order; vertex_index / face_index int32: the
    original index of every survivor; colors rows follow their vertices.  Reads its two counts back once."""
    fn = "mesh.clean"
    mf, md = int(min_faces), float(min_diag)
    if mf != min_faces or mf < 0:
        raise ValueError(f"{fn}: min_faces must be a non-negative integer, got {min_faces!r}")
    if not 0.0 <= md <= 1e150:
        raise ValueError(f"{fn}: min_diag must be a number >= 0, got {min_diag!r}")
    V, F, v, f, c, dev = _mesh_args(fn, vertices, faces, colors)
    i32 = dict(dtype=torch.int32, device=dev)
    if V == 0 or F == 0:
        return CleanMesh(*_empty(dev, c, V), torch.empty(0, **i32), torch.empty(0, **i32))
    lib = _lib.load()
    ws = workspace(lib.goi_mesh_clean_workspace_bytes(V, F), dev)
    counts = torch.empty(3, **i32)
    with torch.cuda.device(dev):
        check(lib.goi_mesh_clean_plan(V, F, ptr(v), ptr(f), mf, md * md, ptr(ws), ptr(counts), stream(dev)))
        nv, nf, st = (int(n) for n in counts.tolist())  # the one read-back: the outputs' sizes (and the status word)
        check_status(st, fn)
        out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((nf, 3), **i32)
        out_c = torch.empty((nv, 3), dtype=torch.float32, device=dev) if c is not None else None
        vidx, fidx = torch.empty(nv, **i32), torch.empty(nf, **i32)
        if nv > 0 or nf > 0:
            check(lib.goi_mesh_clean_emit(V, F, ptr(v), ptr(f), ptr(c), ptr(ws), nv, nf, ptr(out_v), ptr(out_f), ptr(out_c),
                                          ptr(vidx), ptr(fidx), stream(dev)))
    return CleanMesh(out_v, out_f, out_c, vidx, fidx)


def bisect_divisions(count, target, hi=MAX_DIVISIONS) -> int:
    """The divisions decimate(target_faces=target) takes, given count(n) = faces with three distinct cells at n divisions:
    `hi` if count(hi) <= target, otherwise the lower end of a bisection of 1 (count 0) .. hi.  count(result) <= target holds
    although count is not strictly monotone.  At most 1 + ceil(log2(hi - 1)) = 11 calls of count."""
    if count(hi) <= target:
        return hi
    lo = 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count(mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo


def decimate(vertices, faces, colors=None, divisions=None, target_faces=None) -> DecimatedMesh:
    """Vertex clustering on a divisions^3 grid over the box of the members (the module docstring has the arithmetic); give
    exactly one of divisions (2 .. 1024) and target_faces.  A face naming a non-finite vertex is dropped, as is a face whose
    three cells are not distinct and a face whose set of cells repeats that of a lower face; the others keep their order and
    orientation.  Output vertices: the cells a surviving face names, by ascending key, each the mean of its members.
    target_faces: a mesh of no more faces comes back as it is (divisions = 0, cluster = arange; DreamGaussian decimates only a
    larger mesh); otherwise the divisions are bisect_divisions' (1 when even 2 divisions leave too many faces: an empty mesh).
    -> DecimatedMesh(vertices, faces, colors, divisions, cluster int32 [V]: the output vertex of every input vertex or -1).
    Reads back one integer per probe of the bisection, then the two counts once."""
    fn = "mesh.decimate"
    if (divisions is None) == (target_faces is None):
        raise ValueError(f"{fn}: give exactly one of divisions and target_faces")
    if divisions is not None:
        n = int(divisions)
        if n != divisions or not 2 <= n <= MAX_DIVISIONS:
            raise ValueError(f"{fn}: divisions must be an integer in 2 .. {MAX_DIVISIONS}, got {divisions!r}")
    else:
        target = int(target_faces)
        if target != target_faces or target < 0:
            raise ValueError(f"{fn}: target_faces must be a non-negative integer, got {target_faces!r}")
    V, F, v, f, c, dev = _mesh_args(fn, vertices, faces, colors)
    i32 = dict(dtype=torch.int32, device=dev)
    if divisions is None and F <= target:
        return DecimatedMesh(v, f, c, 0, torch.arange(V, **i32))
    if V == 0 or F == 0:
        return DecimatedMesh(*_empty(dev, c, V), divisions if divisions is not None else 1, torch.full((V,), -1, **i32))
    lib = _lib.load()
    ws = workspace(lib.goi_mesh_decimate_workspace_bytes(V, F), dev)
    counts = torch.empty(3, **i32)
    with torch.cuda.device(dev):
        s = stream(dev)
        check(lib.goi_mesh_decimate_members(V, F, ptr(v), ptr(f), ptr(ws), s))
        if divisions is None:
            probe = torch.empty(1, **i32)

            def count(m):
                check(lib.goi_mesh_decimate_probe(V, F, ptr(v), ptr(f), m, ptr(ws), ptr(probe), s))
                return int(probe.item())  # one integer per probe

            n = bisect_divisions(count, target)
        sorted_in = check(lib.goi_mesh_decimate_plan(V, F, ptr(v), ptr(f), n, ptr(ws), ptr(counts), s))
        nv, nf, st = (int(k) for k in counts.tolist())  # the outputs' sizes (and the status word)
        check_status(st, fn)
        out_v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((nf, 3), **i32)
        out_c = torch.empty((nv, 3), dtype=torch.float32, device=dev) if c is not None else None
        cluster = torch.empty(V, **i32)
        check(lib.goi_mesh_decimate_emit(V, F, ptr(v), ptr(c), n, sorted_in, ptr(ws), nv, nf, ptr(out_v), ptr(out_f),
                                         ptr(out_c), ptr(cluster), s))
    return DecimatedMesh(out_v, out_f, out_c, n, cluster)


def vertex_normals(vertices, faces, return_status=False):
    """Mesh.auto_normal: every face adds its un-normalised float32 cross product (v1 - v0) x (v2 - v0) to its three corners; a
    sum with dot <= 1e-20 (an unreferenced vertex, faces that cancel) becomes (0, 0, 1); the sum is divided by
    sqrt(max(dot, 1e-20)).  Where the reference scatter_adds (float atomics on a GPU), each vertex here sums its corners in
    ascending (face, corner) order.  -> float32 [V, 3] (and the status word, a 0-d device tensor, with return_status).  Reads
    nothing back."""
    fn = "mesh.vertex_normals"
    V, F, v, f, _, dev = _mesh_args(fn, vertices, faces)
    lib = _lib.load()
    out = torch.empty((V, 3), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace(lib.goi_mesh_normals_workspace_bytes(V, F), dev)
    with torch.cuda.device(dev):
        check(lib.goi_mesh_normals(V, F, ptr(v), ptr(f), ptr(out), ptr(status), ptr(ws), stream(dev)))
    return (out, status[0]) if return_status else out


def extract(pc, density_thresh=1.0, resolution=128, num_blocks=16, relax_ratio=1.5, selection=None, selection_invert=False,
            colors="rgb", bounds=None, min_opacity=0.005, min_faces=64, min_diag=0.2, target_faces=50000, normals=True) -> Mesh:
    """field.extract_mesh (which takes the field keywords), then clean(min_faces, min_diag), then decimate(target_faces) unless
    target_faces is None or already met (50 000 is DreamGaussian's decimate_target), then vertex_normals.
    -> Mesh(vertices, faces, colors, normals or None, center, scale); save it with io.save_mesh_ply(..., normals=)."""
    raw = field.extract_mesh(pc, density_thresh, resolution, num_blocks, relax_ratio, selection, selection_invert, colors, bounds,
                             min_opacity)
    m = clean(raw.vertices, raw.faces, raw.colors, min_faces, min_diag)
    v, f, c = m.vertices, m.faces, m.colors
    if target_faces is not None and int(f.shape[0]) > int(target_faces):
        v, f, c = decimate(v, f, c, target_faces=target_faces)[:3]
    n = None
    if normals:
        n, status = vertex_normals(v, f, return_status=True)
        check_status(status, "mesh.extract")  # (clean and decimate have read back already: this costs one word)
    return Mesh(v, f, c, n, raw.center, raw.scale)
