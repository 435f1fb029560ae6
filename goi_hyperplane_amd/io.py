"""On-disk formats around the hot path, byte-compatible with the reference so
that scenes, code books and checkpoints move in both directions:

  * point_cloud.ply        scene/gaussian_model.py:255-358 (save_ply / load_ply): binary little-endian
                           PLY, one `vertex` element, float32 properties x y z nx ny nz f_dc_* f_rest_*
                           sem_* opacity scale_* rot_* holding the RAW (pre-activation) parameters
  * semantic_MLP.pt        scene/semantic_model.py:52-63 ({"args", "state_dict"})  -> semantic.SemanticModel
  * LUT.pt                 train.py:189 (torch.save of the [tab_len, ape_dim] Parameter)
  * chkpnt<iter>.pth       train.py:202 + scene/gaussian_model.py:54-90: ((13-tuple), iteration)
  * k-means code-book init train.py:36-56
  * mesh.ply               what field.extract_mesh gives (the reference's "save mesh" button, gui/main.py:607-617): binary
                           little-endian PLY, `vertex` (float x y z, optionally uchar red green blue) and `face`
                           (list uchar int vertex_indices)
  * mesh.obj               what texture.bake gives (the button's mode 'geo+tex', gui/mesh.py:576-622 write_obj): .obj + .mtl +
                           _albedo.png

The reference reads and writes PLY through the `plyfile` package; this module speaks the format
directly with numpy (header grammar of the PLY 1.0 spec: ascii / binary_little_endian /
binary_big_endian, scalar properties).
"""
from __future__ import annotations

import os

import numpy as np
import torch

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def ply_attribute_names(n_dc: int, n_rest: int, n_sem: int, n_scale: int = 3, n_rot: int = 4) -> list:
    """construct_list_of_attributes (scene/gaussian_model.py:255-270)."""
    names = ["x", "y", "z", "nx", "ny", "nz"]
    names += [f"f_dc_{i}" for i in range(n_dc)]
    names += [f"f_rest_{i}" for i in range(n_rest)]
    names += [f"sem_{i}" for i in range(n_sem)]
    names.append("opacity")
    names += [f"scale_{i}" for i in range(n_scale)]
    names += [f"rot_{i}" for i in range(n_rot)]
    return names


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def save_ply(path, xyz, features_dc, features_rest, semantics, opacity, scaling, rotation) -> None:
    """save_ply (scene/gaussian_model.py:272-291).  features_dc [P,1,3], features_rest [P,K,3] in the
    reference's parameter layout; they are written channel-major (transpose(1,2).flatten)."""
    xyz = _np(xyz).astype(np.float32)
    P = xyz.shape[0]
    f_dc = np.ascontiguousarray(np.transpose(_np(features_dc), (0, 2, 1))).reshape(P, -1)
    f_rest = np.ascontiguousarray(np.transpose(_np(features_rest), (0, 2, 1))).reshape(P, -1)
    cols = [xyz, np.zeros_like(xyz), f_dc, f_rest, _np(semantics).reshape(P, -1), _np(opacity).reshape(P, -1),
            _np(scaling).reshape(P, -1), _np(rotation).reshape(P, -1)]
    table = np.ascontiguousarray(np.concatenate([c.astype(np.float32) for c in cols], axis=1), dtype="<f4")
    names = ply_attribute_names(f_dc.shape[1], f_rest.shape[1], cols[4].shape[1], cols[6].shape[1], cols[7].shape[1])
    assert table.shape[1] == len(names)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)  # mkdir_p(os.path.dirname(path))
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % P
    header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())


def read_ply_vertex(path) -> np.ndarray:
    """The first element of a PLY file as a numpy structured array (what plydata.elements[0] gives)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, count, props, in_first = None, None, [], False
        n_elements = 0
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                n_elements += 1
                in_first = n_elements == 1
                if in_first:
                    count = int(tok[2])
            elif tok[0] == "property" and in_first:
                if tok[1] == "list":
                    raise ValueError(f"{path}: list properties are not supported in the vertex element")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt is None or count is None:
            raise ValueError(f"{path}: malformed PLY header")
        if fmt == "ascii":
            rows = np.loadtxt(f, max_rows=count, ndmin=2, dtype=np.float64)
            out = np.empty(count, dtype=[(n, t) for n, t in props])
            for i, (n, _t) in enumerate(props):
                out[n] = rows[:, i]
            return out
        order = {"binary_little_endian": "<", "binary_big_endian": ">"}[fmt]
        dt = np.dtype([(n, order + t) for n, t in props])
        data = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
        return data


REFERENCE_SEM_DIM = 10  # arguments/__init__.py:39 (sem_dim), cuda_rasterizer/config.h:18 (SEM_CHANNELS)


def load_ply(path, max_sh_degree: int = 3, semantic_dim: int | None = None) -> dict:
    """load_ply (scene/gaussian_model.py:308-358): raw parameter arrays in the reference's layout
    (features_dc [P,1,3], features_rest [P,(D+1)^2-1,3]) as float32 numpy arrays.

    semantic_dim=None (default): the semantic features have the width the FILE has (its sem_* columns; a file without
    any gets REFERENCE_SEM_DIM zero columns).  An explicit semantic_dim follows the reference's rule -- a file whose
    number of sem_* columns differs yields ZEROS of the file's width (gaussian_model.py:332-336) -- and warns, because
    decoding or training on those zeros is silent garbage (e.g. a default reference run saves 10 columns)."""
    v = read_ply_vertex(path)
    names = v.dtype.names
    P = v.shape[0]
    xyz = np.stack([v["x"], v["y"], v["z"]], axis=1)
    opacity = np.asarray(v["opacity"])[..., None]
    features_dc = np.zeros((P, 3, 1))
    for c in range(3):
        features_dc[:, c, 0] = v[f"f_dc_{c}"]

    def numbered(prefix):
        return sorted([n for n in names if n.startswith(prefix)], key=lambda x: int(x.split("_")[-1]))

    extra = numbered("f_rest_")
    assert len(extra) == 3 * (max_sh_degree + 1) ** 2 - 3
    features_extra = np.stack([v[n] for n in extra], axis=1).reshape(P, 3, (max_sh_degree + 1) ** 2 - 1) if extra \
        else np.zeros((P, 3, 0))
    sem_names = numbered("sem_")
    want = len(sem_names) if semantic_dim is None else int(semantic_dim)
    sems = np.zeros((P, len(sem_names) or want or REFERENCE_SEM_DIM))
    if len(sem_names) == want:
        for i, n in enumerate(sem_names):
            sems[:, i] = v[n]
    elif sem_names:
        import warnings
        warnings.warn(f"{path}: the file has {len(sem_names)} sem_* columns but semantic_dim={want} was requested; "
                      f"following the reference, the semantic features are ZERO [P,{len(sem_names)}]. Pass "
                      f"semantic_dim=None (or {len(sem_names)}) to load them.", stacklevel=2)
    scales = np.stack([v[n] for n in numbered("scale_")], axis=1)
    rots = np.stack([v[n] for n in numbered("rot")], axis=1)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return {"xyz": f32(xyz), "features_dc": f32(np.transpose(features_dc, (0, 2, 1))),
            "features_rest": f32(np.transpose(features_extra, (0, 2, 1))), "semantics": f32(sems),
            "opacity": f32(opacity), "scaling": f32(scales), "rotation": f32(rots)}


def activate(raw: dict) -> dict:
    """Raw parameters -> what the rasterizer consumes (scene/gaussian_model.py:39-53,90-117:
    exp scaling, sigmoid opacity, normalised rotation, dc + rest concatenated)."""
    t = {k: torch.as_tensor(v) for k, v in raw.items()}
    return {"means3D": t["xyz"], "scales": torch.exp(t["scaling"]),
            "rotations": torch.nn.functional.normalize(t["rotation"]), "opacities": torch.sigmoid(t["opacity"]),
            "shs": torch.cat((t["features_dc"], t["features_rest"]), dim=1), "semantics": t["semantics"]}


# ---- mesh ----------------------------------------------------------------------------------------
def save_mesh_ply(path, vertices, faces, colors=None, normals=None) -> None:
    """A triangle mesh as binary little-endian PLY: element vertex (float x y z, float nx ny nz when normals [V, 3] are given
    (mesh.vertex_normals), and uchar red green blue when colors [V, 3] in [0, 1] are given: round(255 c)), element face (list
    uchar int vertex_indices).  Zero vertices or faces are fine."""
    v = np.ascontiguousarray(_np(vertices), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(_np(faces), dtype="<i4").reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"save_mesh_ply: face indices outside 0 .. {v.shape[0] - 1}")
    vt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        n = np.ascontiguousarray(_np(normals), dtype="<f4").reshape(-1, 3)
        if n.shape[0] != v.shape[0]:
            raise ValueError(f"save_mesh_ply: {n.shape[0]} normals for {v.shape[0]} vertices")
        vt += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        c = np.asarray(_np(colors), dtype=np.float64).reshape(-1, 3)
        if c.shape[0] != v.shape[0]:
            raise ValueError(f"save_mesh_ply: {c.shape[0]} colours for {v.shape[0]} vertices")
        vt += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vrec = np.empty(v.shape[0], dtype=vt)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vrec["nx"], vrec["ny"], vrec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colors is not None:
        c8 = np.rint(np.clip(np.nan_to_num(c), 0.0, 1.0) * 255.0).astype(np.uint8)
        vrec["red"], vrec["green"], vrec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"] = 3
    frec["i"] = f
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % v.shape[0]
    header += "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        header += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % f.shape[0]
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_mesh_ply(path, with_normals=False):
    """-> (vertices float32 [V, 3], faces int32 [F, 3], colors uint8 [V, 3] or None) of a file save_mesh_ply wrote (binary
    little-endian, scalar vertex properties, triangles as `list uchar int`).  with_normals: a fourth item, the file's nx ny nz as
    float32 [V, 3] or None."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property" and elements:
                elements[-1][2].append(tok[1:])
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError(f"{path}: read_mesh_ply reads binary_little_endian files, not {fmt}")
        vertices = faces = colors = normals = None
        for name, count, props in elements:
            if name == "vertex":
                if any(p[0] == "list" for p in props):
                    raise ValueError(f"{path}: list properties are not supported in the vertex element")
                dt = np.dtype([(p[1], "<" + _PLY_TYPES[p[0]]) for p in props])
                rec = np.frombuffer(fh.read(count * dt.itemsize), dtype=dt, count=count)
                vertices = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32).reshape(-1, 3)
                if all(n in rec.dtype.names for n in ("red", "green", "blue")):
                    colors = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1).astype(np.uint8).reshape(-1, 3)
                if all(n in rec.dtype.names for n in ("nx", "ny", "nz")):
                    normals = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1).astype(np.float32).reshape(-1, 3)
            elif name == "face":
                if len(props) != 1 or props[0][0] != "list":
                    raise ValueError(f"{path}: the face element must be one list property")
                dt = np.dtype([("n", "<" + _PLY_TYPES[props[0][1]]), ("i", "<" + _PLY_TYPES[props[0][2]], (3,))])
                rec = np.frombuffer(fh.read(count * dt.itemsize), dtype=dt, count=count)
                if count and not np.all(rec["n"] == 3):
                    raise ValueError(f"{path}: only triangles are supported")
                faces = rec["i"].astype(np.int32).reshape(-1, 3)
            else:
                raise ValueError(f"{path}: unexpected element {name}")
        if vertices is None or faces is None:
            raise ValueError(f"{path}: a mesh needs a vertex and a face element")
        return (vertices, faces, colors, normals) if with_normals else (vertices, faces, colors)


def _write_png_rgb(path, rgb) -> None:
    """uint8 [h, w, 3] as an 8-bit RGB PNG (filter 0 on every row), with zlib and struct alone."""
    import struct
    import zlib
    h, w, _ = rgb.shape
    rows = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, 3 * w)], axis=1)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                 + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def save_mesh_obj(path, textured_mesh) -> None:
    """write_obj (gui/mesh.py:576-622) for a texture.TexturedMesh: `path` (.obj) with `mtllib`, the `v` lines, `vt u 1-v` (1 - v
    in float32), `vn`, `usemtl defaultMat` and `f a/b/c` one-based (vertex / vt / normal indices: faces / ft / faces); the .mtl
    next to it with the reference's lines; <name>_albedo.png = (albedo * 255).astype(uint8) as RGB (albedo clipped to [0, 1]
    first), written with zlib and struct: no image package.  Numbers are printed as Python prints a float32 (the shortest text
    that reads back to the same value).  The reference's .glb writer is not here: pygltflib is not available."""
    if not path.endswith(".obj"):
        raise ValueError(f"save_mesh_obj: {path!r} must end in .obj")
    m = textured_mesh
    v = np.ascontiguousarray(_np(m.vertices), dtype=np.float32).reshape(-1, 3)
    vt = np.ascontiguousarray(_np(m.vt), dtype=np.float32).reshape(-1, 2)
    vn = np.ascontiguousarray(_np(m.normals), dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(_np(m.faces), dtype=np.int64).reshape(-1, 3)
    ft = np.ascontiguousarray(_np(m.ft), dtype=np.int64).reshape(-1, 3)
    if ft.shape != f.shape or vn.shape != v.shape:
        raise ValueError("save_mesh_obj: faces / ft and vertices / normals must have matching shapes")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0] or ft.min() < 0 or ft.max() >= vt.shape[0]):
        raise ValueError("save_mesh_obj: an index outside its array")
    albedo = np.asarray(_np(m.albedo), dtype=np.float32)
    if albedo.ndim != 3 or albedo.shape[2] != 3:
        raise ValueError("save_mesh_obj: albedo must be [h, w, 3]")
    mtl_path, albedo_path = path[:-4] + ".mtl", path[:-4] + "_albedo.png"
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    one = np.float32(1)
    lines = [f"mtllib {os.path.basename(mtl_path)} \n"]
    lines += [f"v {p[0]} {p[1]} {p[2]} \n" for p in v]
    lines += [f"vt {p[0]} {one - p[1]} \n" for p in vt]
    lines += [f"vn {p[0]} {p[1]} {p[2]} \n" for p in vn]
    lines.append("usemtl defaultMat \n")
    lines += [f"f {a[0] + 1}/{b[0] + 1}/{a[0] + 1} {a[1] + 1}/{b[1] + 1}/{a[1] + 1} {a[2] + 1}/{b[2] + 1}/{a[2] + 1} \n"
              for a, b in zip(f.tolist(), ft.tolist())]
    with open(path, "w") as fp:
        fp.writelines(lines)
    with open(mtl_path, "w") as fp:
        fp.write("newmtl defaultMat \nKa 1 1 1 \nKd 1 1 1 \nKs 0 0 0 \nTr 1 \nillum 1 \nNs 0 \n"
                 f"map_Kd {os.path.basename(albedo_path)} \n")
    _write_png_rgb(albedo_path, (np.clip(np.nan_to_num(albedo), 0.0, 1.0) * 255).astype(np.uint8))


def read_mesh_obj(path) -> dict:
    """A file save_mesh_obj wrote -> {"vertices" float32 [V, 3], "vt" float32 [Nt, 2] AS PRINTED (u, 1 - v), "normals" float32
    [Nn, 3], "faces", "ft", "fn" int32 [F, 3] zero-based, "mtllib", "usemtl", "mtl": the .mtl file's lines as {key: text}}."""
    rows = {"v": [], "vt": [], "vn": []}
    tri, names = [], {"mtllib": None, "usemtl": None}
    with open(path) as fp:
        for line in fp:
            tok = line.split()
            if not tok:
                continue
            if tok[0] in rows:
                rows[tok[0]].append([float(t) for t in tok[1:]])
            elif tok[0] == "f":
                if len(tok) != 4:
                    raise ValueError(f"{path}: only triangles are supported")
                tri.append([[int(i) - 1 for i in t.split("/")] for t in tok[1:]])
            elif tok[0] in names:
                names[tok[0]] = tok[1]
    t = np.asarray(tri, dtype=np.int32).reshape(-1, 3, 3)
    out = {"vertices": np.asarray(rows["v"], dtype=np.float32).reshape(-1, 3), "vt": np.asarray(rows["vt"], dtype=np.float32).reshape(-1, 2),
           "normals": np.asarray(rows["vn"], dtype=np.float32).reshape(-1, 3), "faces": t[:, :, 0], "ft": t[:, :, 1], "fn": t[:, :, 2]}
    out.update(names)
    out["mtl"] = {}
    if names["mtllib"]:
        with open(os.path.join(os.path.dirname(path), names["mtllib"])) as fp:
            for line in fp:
                tok = line.split()
                if tok:
                    out["mtl"][tok[0]] = " ".join(tok[1:])
    return out


# ---- code book -----------------------------------------------------------------------------------
def save_codebook(directory, semantic_mlp, lut) -> None:
    """train.py:187-189: semantic_MLP.pt + LUT.pt next to point_cloud.ply."""
    os.makedirs(directory, exist_ok=True)
    semantic_mlp.save(os.path.join(directory, "semantic_MLP.pt"))
    torch.save(lut, os.path.join(directory, "LUT.pt"))


def load_codebook(directory, map_location=None):
    """gui/gs_renderer.py:214-228."""
    from .semantic import SemanticModel
    mlp = SemanticModel.load(os.path.join(directory, "semantic_MLP.pt"), map_location=map_location)
    lut = torch.load(os.path.join(directory, "LUT.pt"), map_location=map_location)
    return mlp, lut


def kmeans(x: torch.Tensor, ncluster: int, niter: int = 10) -> torch.Tensor:
    """train.py:36-56: spherical k-means used to initialise the code book.  Same RNG consumption
    (one randperm for the seeds, one per iteration for dead clusters) and the same in-place
    normalisation of `x`; the per-cluster means are one index_add instead of `ncluster` masked means."""
    N, D = x.size()
    x /= x.norm(dim=1, keepdim=True)
    centers = x[torch.randperm(N)[:ncluster]]
    for _ in range(niter):
        centers = centers / centers.norm(dim=1, keepdim=True)
        assignments = (x @ centers.T).argmax(1)
        sums = torch.zeros((ncluster, D), dtype=x.dtype, device=x.device).index_add_(0, assignments, x)
        counts = torch.bincount(assignments, minlength=ncluster).to(x.dtype)
        centers = sums / counts[:, None]  # empty cluster -> 0/0 = nan, like the mean of an empty selection
        nanix = torch.any(torch.isnan(centers), dim=1)
        ndead = int(nanix.sum().item())
        centers[nanix] = x[torch.randperm(N)[:ndead]]
    return centers


# ---- checkpoint ------------------------------------------------------------------------------------
CHECKPOINT_FIELDS = ("active_sh_degree", "xyz", "features_dc", "features_rest", "semantics", "scaling", "rotation",
                     "opacity", "max_radii2D", "xyz_gradient_accum", "denom", "optimizer_state", "spatial_lr_scale")


def save_checkpoint(path, model: dict, iteration: int) -> None:
    """train.py:202: torch.save((gaussians.capture(), iteration), path); capture() is the 13-tuple of
    scene/gaussian_model.py:54-69 in CHECKPOINT_FIELDS order."""
    torch.save((tuple(model[k] for k in CHECKPOINT_FIELDS), iteration), path)


def load_checkpoint(path, map_location=None):
    """-> (dict keyed by CHECKPOINT_FIELDS, iteration)  (train.py:72-73, gaussian_model.py:71-88)."""
    model_params, iteration = torch.load(path, map_location=map_location, weights_only=False)
    if len(model_params) != len(CHECKPOINT_FIELDS):
        raise ValueError(f"{path}: expected a {len(CHECKPOINT_FIELDS)}-tuple, got {len(model_params)}")
    return dict(zip(CHECKPOINT_FIELDS, model_params)), iteration
