"""Texture bake for a mesh on the device (csrc/texture.hip): the second mode of the reference's "save mesh"
button, save_model(mode='geo+tex') of gui/main.py:614-752, which there needs xatlas, nvdiffrast, scipy and sklearn.

    atlas           a per-face UV atlas in place of Mesh.auto_uv (xatlas): a function of (F, size) alone
    orbit_cameras   the 26 views of main.py:632-633 (orbit_camera + MiniCam) as scene.Camera-compatible objects
    clip_positions  vertices through a camera's full_proj_transform, elementwise (no GEMM: the same bits every run)
    rasterize       a z-buffer triangle rasterizer (what dr.rasterize supplied)
    resolve         the three dr.interpolate calls and main.py:682-704: uv, normal, view cosine, mask, colour per pixel
    grid_put        mipmap_linear_grid_put_2d (gui/grid_put.py:129-159) without float atomics
    accumulate      main.py:718-720: a texel takes a view only while its count is < 0.1;  normalize: main.py:722-723
    fill            main.py:730-749: the margin around the charts takes the nearest chart texel
    bake            all of it -> TexturedMesh; save it with io.save_mesh_obj

All functions take device tensors and run on the current stream; there is no CPU fallback.  Nothing accumulates floats with
atomics, so every result is bit-identical from run to run; tests/texture_reference.py restates every function in numpy with
one float32 rounding per operation, and the tests compare bits.  Read-backs: none of atlas, clip_positions, rasterize,
resolve, grid_put, accumulate, normalize and fill reads anything back (no output's size depends on the data; look at the
`status` words where you read results back); bake reads one status word back after its last view, none inside the view loop.

The atlas, which is part of the contract.  Texel i of a `size`-wide texture sits at uv = i / (size - 1) (grid_put's
convention); u runs along the columns, v along the rows.  pairs = ceil(F / 2), n = ceil(sqrt(pairs)) (1 for F = 0), cell =
size // n texels (ValueError under 4).  Faces 2 p and 2 p + 1 share the cell in row p // n, column p % n, whose first texel is
(x0, y0) = (cell * (p % n), cell * (p // n)).  In texel units relative to (x0, y0), corner k of the face being vertex k:
    face 2 p      (0.5, 0.5)  (c - 2.5, 0.5)  (0.5, c - 2.5)              [c = cell]
    face 2 p + 1  (c - 1.5, c - 1.5)  (1.5, c - 1.5)  (c - 1.5, 1.5)
and vt = (x0 + x, y0 + y) / (size - 1), one float32 division.  Both triangles have positive area, stay half a texel inside
the square of their cell's texel centres [x0, x0 + c - 1]^2, and their hypotenuses x + y = c - 2 and x + y = c are one texel
apart in the maximum norm; triangles of neighbouring cells are two texels apart.

The rasterizer, which is part of the contract.  For a vertex (x, y, z, w): sx = ((x / w + 1) * W - 1) * 0.5, sy likewise with
H (pixel centres at integers: the Gaussian rasterizer's ndc2Pix), X = rint(sx * 256), Y = rint(sy * 256) (half to even).  A
face with an index outside [0, V), a w <= 0 (nvdiffrast clips; the cameras here orbit outside the mesh), a |sx| or |sy| that
is not <= 2^20, or twice-area a = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) = 0 draws nothing; there is no back-face culling.
e_k at pixel (px, py), for the edge from vertex k + 1 to vertex k + 2 (mod 3) with d = s (P_{k+2} - P_{k+1}), s = sign(a):
e_k = dx (256 py - Y_{k+1}) - dy (256 px - X_{k+1}), all int64.  The pixel is covered when every e_k > 0, or e_k = 0 and
(dy > 0 or (dy = 0 and dx < 0)).  s_k = float(e_k) / float(|a|); p_k = s_k / w_k; sum = (p0 + p1) + p2; u = p0 / sum; v = p1 /
sum; r = (1 - u) - v; zw = ((u z0 + v z1) + r z2) / ((u w0 + v w1) + r w2).  The smallest zw wins (a NaN draws nothing), equal
bits go to the lower face.  tri = face + 1 (0: empty), bary = (u, v), zw; zeros where empty.

resolve interpolates as (u a0 + v a1) + r a2 with r = (1 - u) - v.  grid_put sums every texel's taps in ascending (tap 00,
01, 10, 11; sample) order -- the order of the reference's four sequential scatter_adds on the CPU -- and upsamples a level as
upsample_bilinear2d(align_corners=False) does: scale = in / out, src = max(scale * (dst + 0.5) - 0.5, 0), i0 = int(src), i1 =
i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, value = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).  A texel's
run is summed by one lane, so a pathological view that sends every sample to one texel is slow, not wrong.  fill's ties go
to the smaller squared distance, then the smaller row, then the smaller column (sklearn's choice is arbitrary).

Departures from the reference: the per-face atlas (no xatlas); no clipping of faces that cross w = 0; the early exit of
mipmap_linear_grid_put_2d (a host synchronisation; adding under an all-false mask is a no-op) is dropped; orbit_cameras
converts the OpenGL pose to the rasterizer's convention (rows 1 and 2 of the world-to-camera matrix negated, which the
reference's MiniCam has commented out: its camera looks away from the orbit's target), rectify=False gives the reference's.
"""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, scene
from ._lib import check, ptr, stream, workspace
from .field import _f32

# GOI_TEXTURE_* of include/goi_raster.h
STATUS_SORT, STATUS_RANGE = 2, 8
MAX_CHANNELS, MAX_RADIUS, MAX_SIZE = 4, 127, 16384
MIN_CELL = 4
_NO_CPU = "goi_hyperplane_amd.texture: tensors must live on a ROCm GPU; there is no CPU fallback"

Atlas = namedtuple("Atlas", "vt ft vmapping")
Atlas.__doc__ = """vt float32 [3 F, 2], ft int32 [F, 3] = arange(3 F).view(F, 3), vmapping = faces.view(-1) (None when atlas() was
not given the faces): vertices[vmapping] and normals[vmapping] with ft as faces is Mesh.align_v_to_vt, a gather."""
Raster = namedtuple("Raster", "tri bary zw status")
Raster.__doc__ = """tri int32 [H, W]: face + 1, 0 where empty; bary float32 [H, W, 2]: the perspective-correct weights of the face's
vertices 0 and 1; zw float32 [H, W]: z / w; status: int32 0-d device tensor of STATUS_* bits."""
TexturedMesh = namedtuple("TexturedMesh", "vertices faces vt ft normals albedo mask")
TexturedMesh.__doc__ = """vertices float32 [3 F, 3], faces = ft int32 [F, 3], vt float32 [3 F, 2], normals float32 [3 F, 3], albedo
float32 [h, w, 3] in [0, 1], mask bool [h, w]: the texels a view reached (the others are filled or zero)."""

VERS = [0] * 8 + [-45] * 8 + [45] * 8 + [-89.9, 89.9]  # gui/main.py:632-633
HORS = [0, 45, -45, 90, -90, 135, -135, 180] * 3 + [0, 0]


def _on_device(fn, *tensors):
    used = [t for t in tensors if t is not None]
    if not all(isinstance(t, torch.Tensor) for t in used):
        raise ValueError(f"{fn}: every argument must be a tensor")
    if not all(t.is_cuda for t in used):
        raise RuntimeError(_NO_CPU)
    if any(t.device != used[0].device for t in used):
        raise ValueError(f"{fn}: all tensors must live on one device")
    return used[0].device


def _size(fn, name, n, lo=1, hi=MAX_SIZE):
    k = int(n)
    if k != n or not lo <= k <= hi:
        raise ValueError(f"{fn}: {name} must be an integer in {lo} .. {hi}, got {n!r}")
    return k


def _faces(fn, name, f):
    if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[1] != 3 or f.dtype != torch.int32:
        raise ValueError(f"{fn}: {name} must be an int32 [F, 3] tensor")
    return f.detach().contiguous()


def check_status(status, fn="texture") -> None:
    """Raises for a non-zero status word (this reads it back)."""
    st = int(status)
    if st & STATUS_RANGE:
        raise ValueError(f"{fn}: an index outside its array (a face naming a vertex that is not there)")
    if st:
        raise RuntimeError(f"{fn}: a sort timed out (status {st}); the result is not usable")


# ---- atlas ------------------------------------------------------------------------------------------------------------------
def atlas_grid(n_faces, size):
    """(n, cell) of the module docstring's layout; ValueError when a cell would be under MIN_CELL texels."""
    F, S = int(n_faces), int(size)
    if F != n_faces or F < 0:
        raise ValueError(f"texture.atlas: n_faces must be a non-negative integer, got {n_faces!r}")
    _size("texture.atlas", "size", size, 2)
    pairs = (F + 1) // 2
    n = math.isqrt(pairs - 1) + 1 if pairs > 0 else 1
    cell = S // n
    if cell < MIN_CELL:
        raise ValueError(f"texture.atlas: {F} faces need {n} x {n} cells, {cell} texels each in a {S}-texel texture; a cell "
                         f"must have at least {MIN_CELL} (use a larger texture or decimate further)")
    return n, cell


def atlas(n_faces, size, faces=None, device=None) -> Atlas:
    """The per-face atlas of the module docstring for F = n_faces faces in a size x size texture.  faces (int32 [F, 3]): fills
    vmapping = faces.view(-1) and gives the device.  Plain index arithmetic, a function of (F, size) alone."""
    n, cell = atlas_grid(n_faces, size)
    F, S = int(n_faces), int(size)
    if faces is not None:
        if tuple(faces.shape) != (F, 3):
            raise ValueError(f"texture.atlas: faces must be [{F}, 3], got {tuple(faces.shape)}")
        device = faces.device
    f = torch.arange(F, dtype=torch.int64, device=device)
    p, odd = f // 2, (f % 2).bool()
    x0, y0 = (cell * (p % n)).double(), (cell * (p // n)).double()
    c = float(cell)
    lower = torch.tensor([[0.5, 0.5], [c - 2.5, 0.5], [0.5, c - 2.5]], dtype=torch.float64, device=device)
    upper = torch.tensor([[c - 1.5, c - 1.5], [1.5, c - 1.5], [c - 1.5, 1.5]], dtype=torch.float64, device=device)
    local = torch.where(odd[:, None, None], upper[None], lower[None])  # [F, 3, 2]
    texel = local + torch.stack([x0, y0], dim=1)[:, None, :]  # multiples of 0.5 far below 2^24: exact in float32 too
    vt = (texel.float() / torch.tensor(float(S - 1), dtype=torch.float32, device=device)).reshape(3 * F, 2)
    ft = torch.arange(3 * F, dtype=torch.int32, device=device).view(F, 3)
    return Atlas(vt, ft, None if faces is None else faces.reshape(-1))


# ---- cameras ----------------------------------------------------------------------------------------------------------------
@dataclass
class OrbitView(scene.Camera):
    """scene.Camera plus `pose`, the OpenGL camera-to-world matrix of orbit_camera (float32 [4, 4]); resolve wants pose[:3, :3]."""
    pose: np.ndarray = None


def _safe_normalize(x, eps=1e-20):
    return x / np.sqrt(np.maximum(np.sum(x * x, axis=-1, keepdims=True), eps))


def orbit_pose(elevation, azimuth, radius=1.0) -> np.ndarray:
    """orbit_camera(elevation, azimuth, radius) of gui/cam_utils.py:105-143 (degrees, target the origin, OpenGL): float32 [4, 4]."""
    el, az = np.deg2rad(elevation), np.deg2rad(azimuth)
    x = radius * np.cos(el) * np.sin(az)
    y = -radius * np.sin(el)
    z = radius * np.cos(el) * np.cos(az)
    campos = np.array([x, y, z]) + np.zeros([3], dtype=np.float32)
    forward = _safe_normalize(campos - np.zeros([3], dtype=np.float32))
    up = np.array([0, 1, 0], dtype=np.float32)
    right = _safe_normalize(np.cross(up, forward))
    up = _safe_normalize(np.cross(forward, right))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.stack([right, up, forward], axis=1)
    T[:3, 3] = campos
    return T


def orbit_cameras(resolution=512, radius=2.0, fovy=60.0, vers=None, hors=None, znear=0.01, zfar=100.0, rectify=True) -> list:
    """The views of gui/main.py:632-657: orbit_pose(ver, hor, radius) through MiniCam (gui/gs_renderer.py:143-169) at
    resolution^2, fovy in degrees (OrbitCamera's default 60; fovx follows from the square image), as OrbitView objects.
    rectify=True negates rows 1 and 2 of the world-to-camera matrix (OpenGL's -z forward, +y up to the rasterizer's +z forward,
    +y down) so that the camera sees the orbit's target, and camera_center is the camera's position; rectify=False is the
    reference's MiniCam as it stands (inv(pose) as it is, camera_center = -position), which looks away from the target  (Not
    DreamGaussian's w2c[1:3, :3] *= -1; w2c[:3, 3] *= -1 either: that also negates the x translation, which agrees only for a
    target on the camera's axis; whole rows are the consistent form for a target off the origin.)"""
    vers = VERS if vers is None else list(vers)
    hors = HORS if hors is None else list(hors)
    if len(vers) != len(hors):
        raise ValueError("texture.orbit_cameras: vers and hors must have the same length")
    res = _size("texture.orbit_cameras", "resolution", resolution)
    fy = float(np.deg2rad(fovy))
    fx = float(2 * np.arctan(np.tan(fy / 2) * res / res))
    proj = np.zeros((4, 4), dtype=np.float32)  # getProjectionMatrix (gs_renderer.py:127-140)
    proj[0, 0] = 1 / math.tan(fx / 2)
    proj[1, 1] = 1 / math.tan(fy / 2)
    proj[3, 2] = 1.0
    proj[2, 2] = zfar / (zfar - znear)
    proj[2, 3] = -(zfar * znear) / (zfar - znear)
    out = []
    for ver, hor in zip(vers, hors):
        pose = orbit_pose(ver, hor, radius)
        w2c = np.linalg.inv(pose)
        if rectify:
            w2c[1:3, :] *= -1
        view_T = np.ascontiguousarray(w2c.T, dtype=np.float32)
        full = (view_T @ np.ascontiguousarray(proj.T)).astype(np.float32)
        center = pose[:3, 3].copy() if rectify else -pose[:3, 3]
        out.append(OrbitView(res, res, fx, fy, view_T, full, center.astype(np.float32), pose))
    return out


def clip_positions(vertices, full_proj_transform):
    """[V, 3] vertices through a camera's full_proj_transform M ([4, 4], row vectors: clip = (x, y, z, 1) @ M) as
    ((x M[0] + y M[1]) + z M[2]) + M[3], elementwise float32 with one rounding per operation -> [V, 4]."""
    v, m = vertices, full_proj_transform
    return ((v[:, 0:1] * m[0] + v[:, 1:2] * m[1]) + v[:, 2:3] * m[2]) + m[3]


# ---- rasterize / resolve ----------------------------------------------------------------------------------------------------
def rasterize(v_clip, faces, H, W) -> Raster:
    """v_clip float32 [V, 4] clip-space positions, faces int32 [F, 3] -> Raster at H x W; the module docstring has the
    arithmetic.  Reads nothing back."""
    fn = "texture.rasterize"
    H, W = _size(fn, "H", H), _size(fn, "W", W)
    f = _faces(fn, "faces", faces)
    if not isinstance(v_clip, torch.Tensor) or v_clip.dim() != 2 or v_clip.shape[1] != 4:
        raise ValueError(f"{fn}: v_clip must be a [V, 4] tensor")
    V, F = int(v_clip.shape[0]), int(f.shape[0])
    v = _f32(fn, "v_clip", v_clip, (V, 4)).detach().contiguous()
    if V >= 2 ** 30 or 3 * F >= 2 ** 30:
        raise ValueError(f"{fn}: need V < 2^30 and 3 F < 2^30")
    dev = _on_device(fn, v, f)
    lib = _lib.load()
    tri = torch.empty((H, W), dtype=torch.int32, device=dev)
    bary = torch.empty((H, W, 2), dtype=torch.float32, device=dev)
    zw = torch.empty((H, W), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace(lib.goi_texture_rasterize_workspace_bytes(F, H, W), dev)
    with torch.cuda.device(dev):
        check(lib.goi_texture_rasterize(V, F, ptr(v), ptr(f), H, W, ptr(tri), ptr(bary), ptr(zw), ptr(status), ptr(ws),
                                        stream(dev)))
    return Raster(tri, bary, zw, status[0])


def resolve(raster, vt, ft, vn, faces, pose_rot, image, return_status=False):
    """Per pixel of `raster`: uv = vt [Nt, 2] through ft, n = vn [Nn, 3] through faces, both interpolated with the raster's
    barycentrics; n / sqrt(max(n.n, 1e-20)); viewcos = (n @ pose_rot)[2] = (n0 R02 + n1 R12) + n2 R22 (pose_rot float32 [3, 3],
    the camera pose's rotation); -> coords float32 [H W, 2] = clamp(uv, 0, 1)[[1, 0]] * 2 - 1 (zeros where the pixel is empty),
    values float32 [H W, 3] = image [3, H, W] per pixel, valid bool [H W] = tri > 0 and viewcos > 0.5.  Invalid pixels stay in
    place: nothing is compacted and nothing is read back."""
    fn = "texture.resolve"
    H, W = (int(s) for s in raster.tri.shape)
    ft_c, f_c = _faces(fn, "ft", ft), _faces(fn, "faces", faces)
    F = int(f_c.shape[0])
    if int(ft_c.shape[0]) != F:
        raise ValueError(f"{fn}: ft and faces must have the same number of rows")
    nt, nn = int(vt.shape[0]), int(vn.shape[0])
    vt_c = _f32(fn, "vt", vt, (nt, 2)).detach().contiguous()
    vn_c = _f32(fn, "vn", vn, (nn, 3)).detach().contiguous()
    rot = _f32(fn, "pose_rot", pose_rot, (3, 3)).detach().contiguous()
    img = _f32(fn, "image", image, (3, H, W)).detach().contiguous()
    tri, bary = raster.tri.contiguous(), raster.bary.contiguous()
    dev = _on_device(fn, tri, bary, vt_c, ft_c, vn_c, f_c, rot, img)
    lib = _lib.load()
    coords = torch.empty((H * W, 2), dtype=torch.float32, device=dev)
    values = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
    valid = torch.empty(H * W, dtype=torch.bool, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.goi_texture_resolve(nt, nn, F, H, W, ptr(tri), ptr(bary), ptr(vt_c), ptr(ft_c), ptr(vn_c), ptr(f_c), ptr(rot),
                                      ptr(img), ptr(coords), ptr(values), ptr(valid), ptr(status), stream(dev)))
    return (coords, values, valid, status[0]) if return_status else (coords, values, valid)


# ---- grid put ---------------------------------------------------------------------------------------------------------------
def _grid_put(fn, H, W, coords, values, valid, min_resolution, acc=None, norm=False):
    """-> (result, count, status) and, with norm (which needs acc = (albedo, cnt)), normalize(albedo, cnt) after the view was
    accumulated, from the same kernel: (result, count, status, out, mask)."""
    H, W = _size(fn, "H", H), _size(fn, "W", W)
    mr = _size(fn, "min_resolution", min_resolution, 1, 2 ** 30)
    if not isinstance(values, torch.Tensor) or values.dim() != 2 or not 1 <= values.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"{fn}: values must be [N, C] with 1 <= C <= {MAX_CHANNELS}")
    N, Cn = int(values.shape[0]), int(values.shape[1])
    if N >= 2 ** 28:
        raise ValueError(f"{fn}: need N < 2^28")
    co = _f32(fn, "coords", coords, (N, 2)).detach().contiguous()
    va = _f32(fn, "values", values, (N, Cn)).detach().contiguous()
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (N,):
            raise ValueError(f"{fn}: valid must be a bool or uint8 [N] tensor")
        valid = valid.detach().contiguous()
    if acc is not None:  # (albedo [H, W, C], cnt with H W elements), updated in place
        ah, aw, ac_ = _texture_pair(fn, *acc)
        if (ah, aw, ac_) != (H, W, Cn) or not acc[0].is_contiguous() or not acc[1].is_contiguous():
            raise ValueError(f"{fn}: the accumulated texture must be contiguous [{H}, {W}, {Cn}]")
    dev = _on_device(fn, co, va, valid, *(acc or ()))
    lib = _lib.load()
    result = torch.empty((H, W, Cn), dtype=torch.float32, device=dev)
    count = torch.empty((H, W, 1), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace(lib.goi_texture_grid_put_workspace_bytes(N, Cn, H, W), dev)
    a, ac = acc if acc is not None else (None, None)
    out = torch.empty_like(a) if norm else None
    mask = torch.empty((H, W), dtype=torch.bool, device=dev) if norm else None
    with torch.cuda.device(dev):
        check(lib.goi_texture_grid_put(N, Cn, H, W, mr, ptr(co), ptr(va), ptr(valid), ptr(result), ptr(count), ptr(a), ptr(ac),
                                       ptr(out), ptr(mask), ptr(status), ptr(ws), stream(dev)))
    return (result, count, status[0], out, mask) if norm else (result, count, status[0])


def grid_put(H, W, coords, values, valid=None, min_resolution=32, return_count=False, return_status=False):
    """mipmap_linear_grid_put_2d(H, W, coords [N, 2] in [-1, 1], values [N, C], min_resolution, return_count): for every level
    H, H / 2, ... while min(level) > min_resolution, linear_grid_put_2d's four-tap splat (its clamp of the base index to 0 ..
    level - 2 included), upsampled to H x W and added where the running count is exactly 0.  valid (bool [N]): the samples that
    take part (a sample with a non-finite coordinate takes no part either).  -> result [H, W, C] divided by the count where it
    is > 0, or (result, count [H, W, 1]) undivided with return_count; with return_status the status word follows.  Reads
    nothing back."""
    result, count, status = _grid_put("texture.grid_put", H, W, coords, values, valid, min_resolution)
    out = (result, count) if return_count else (normalize(result, count)[0],)
    if return_status:
        out = out + (status,)
    return out if len(out) > 1 else out[0]


def _texture_pair(fn, albedo, cnt):
    if not isinstance(albedo, torch.Tensor) or albedo.dim() != 3 or not 1 <= albedo.shape[2] <= MAX_CHANNELS:
        raise ValueError(f"{fn}: the texture must be [h, w, C] with 1 <= C <= {MAX_CHANNELS}")
    h, w, Cn = (int(s) for s in albedo.shape)
    _f32(fn, "the texture", albedo, (h, w, Cn))
    if not isinstance(cnt, torch.Tensor) or cnt.dtype != torch.float32 or cnt.numel() != h * w:
        raise ValueError(f"{fn}: the count must be float32 with {h} x {w} elements")
    return h, w, Cn


def accumulate(albedo, cnt, cur_albedo, cur_cnt) -> None:
    """gui/main.py:718-720, in place: where cnt < 0.1, albedo += cur_albedo and cnt += cur_cnt (the first view to reach a texel
    wins it).  albedo, cur_albedo float32 [h, w, C]; cnt, cur_cnt float32 [h, w] or [h, w, 1]; albedo and cnt contiguous."""
    fn = "texture.accumulate"
    h, w, Cn = _texture_pair(fn, albedo, cnt)
    _texture_pair(fn, cur_albedo, cur_cnt)
    if tuple(cur_albedo.shape) != (h, w, Cn):
        raise ValueError(f"{fn}: the two textures must have one shape")
    if not albedo.is_contiguous() or not cnt.is_contiguous():
        raise ValueError(f"{fn}: albedo and cnt are updated in place and must be contiguous")
    dev = _on_device(fn, albedo, cnt, cur_albedo, cur_cnt)
    cur, cc = cur_albedo.detach().contiguous(), cur_cnt.detach().contiguous()
    with torch.cuda.device(dev):
        check(_lib.load().goi_texture_accumulate(h * w, Cn, ptr(albedo), ptr(cnt), ptr(cur), ptr(cc), stream(dev)))


def normalize(albedo, cnt):
    """gui/main.py:722-723: mask = cnt > 0; albedo / cnt where mask, albedo elsewhere -> (float32 [h, w, C], bool [h, w])."""
    fn = "texture.normalize"
    h, w, Cn = _texture_pair(fn, albedo, cnt)
    dev = _on_device(fn, albedo, cnt)
    a, c = albedo.detach().contiguous(), cnt.detach().contiguous()
    out = torch.empty_like(a)
    mask = torch.empty((h, w), dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        check(_lib.load().goi_texture_normalize(h * w, Cn, ptr(a), ptr(c), ptr(out), ptr(mask), stream(dev)))
    return out, mask


# ---- fill -------------------------------------------------------------------------------------------------------------------
def fill(albedo, mask, radius=32, return_index=False):
    """gui/main.py:730-749 on the device.  The inpaint region -- binary_dilation(mask, iterations=radius) minus mask, scipy's
    default 4-neighbour cross -- is the texels outside `mask` within L1 distance `radius` of it; each takes the colour of its
    nearest mask texel (Euclidean; ties: the smaller row, then the smaller column), which is what the reference's kd-tree over
    mask minus its 3-step erosion finds.  albedo float32 [h, w, C], mask bool [h, w], 0 <= radius <= 127 -> the filled texture;
    with return_index also int32 [h, w]: the flat index of the texel each inpaint texel took, -1 outside the region.  Reads
    nothing back."""
    fn = "texture.fill"
    if not isinstance(albedo, torch.Tensor) or albedo.dim() != 3 or not 1 <= albedo.shape[2] <= MAX_CHANNELS:
        raise ValueError(f"{fn}: albedo must be [h, w, C] with 1 <= C <= {MAX_CHANNELS}")
    h, w, Cn = (int(s) for s in albedo.shape)
    _size(fn, "h", h), _size(fn, "w", w)
    R = _size(fn, "radius", radius, 0, MAX_RADIUS)
    a = _f32(fn, "albedo", albedo, (h, w, Cn)).detach().contiguous()
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (h, w):
        raise ValueError(f"{fn}: mask must be a bool or uint8 [{h}, {w}] tensor")
    m = mask.detach().contiguous()
    dev = _on_device(fn, a, m)
    lib = _lib.load()
    out = torch.empty_like(a)
    nearest = torch.empty((h, w), dtype=torch.int32, device=dev)
    ws = workspace(lib.goi_texture_fill_workspace_bytes(h, w), dev)
    with torch.cuda.device(dev):
        check(lib.goi_texture_fill(h, w, Cn, R, ptr(a), ptr(m), ptr(out), ptr(nearest), ptr(ws), stream(dev)))
    return (out, nearest) if return_index else out


# ---- bake -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def bake(pc, mesh, bg_color, texture_size=1024, render_resolution=512, cameras=None, radius=2.0, fovy=60.0, fill_radius=32,
         min_resolution=None) -> TexturedMesh:
    """save_model(mode='geo+tex') behind extract_mesh: atlas -> vertices and normals gathered by vmapping -> per camera
    render.render_gui(camera, pc, bg_color), rasterize the mesh with the same camera's full_proj_transform (so mesh pixels and
    Gaussian pixels coincide), resolve, grid_put(min_resolution, return_count=True) with accumulate folded into its last
    kernel (and, for the last view, normalize too) -> fill(fill_radius).  min_resolution None: texture_size // 4, the reference's 256 at its 1024 (two
    levels; a fixed 256 would leave a smaller texture without any level, that is empty).  mesh: anything with vertices, faces and normals (mesh.extract's Mesh; normals None:
    mesh.vertex_normals); cameras None: orbit_cameras(render_resolution, radius, fovy), otherwise OrbitView-like objects (a
    scene.Camera plus `pose`).  No host synchronisation inside the view loop: every camera matrix is uploaded before it, and
    the status words are read back once, after the last view."""
    from . import mesh as mesh_mod
    from . import render
    fn = "texture.bake"
    faces = _faces(fn, "mesh.faces", mesh.faces)
    dev = _on_device(fn, mesh.vertices, faces)
    F = int(faces.shape[0])
    h = w = _size(fn, "texture_size", texture_size, 2)
    if min_resolution is None:
        min_resolution = max(h // 4, 1)
    at = atlas(F, h, faces=faces)
    normals = mesh.normals if getattr(mesh, "normals", None) is not None else mesh_mod.vertex_normals(mesh.vertices, faces)
    idx = at.vmapping.long()
    v, vn = mesh.vertices[idx].contiguous(), normals[idx].contiguous()
    if cameras is None:
        cameras = orbit_cameras(render_resolution, radius, fovy)
    views = [(render.TorchCamera(c, dev), torch.tensor(np.ascontiguousarray(c.pose[:3, :3], dtype=np.float32), device=dev))
             for c in cameras]
    albedo = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros((h, w, 1), dtype=torch.float32, device=dev)
    status = torch.zeros((), dtype=torch.int32, device=dev)
    out = mask = None
    for k, (cam, rot) in enumerate(views):
        image = render.render_gui(cam, pc, bg_color)["image"]
        r = rasterize(clip_positions(v, cam.full_proj_transform), at.ft, cam.image_height, cam.image_width)
        coords, values, valid, st = resolve(r, at.vt, at.ft, vn, at.ft, rot, image, return_status=True)
        put = _grid_put(fn, h, w, coords, values, valid, min_resolution, acc=(albedo, cnt), norm=k == len(views) - 1)
        status = status | r.status | st | put[2]
        out, mask = put[3:] if len(put) > 3 else (None, None)  # the last view's kernel normalizes as well
    if out is None:  # no camera at all
        out, mask = normalize(albedo, cnt)
    out = fill(out, mask, fill_radius)
    check_status(status, fn)  # the one read-back
    return TexturedMesh(v, at.ft, at.vt, at.ft, vn, out, mask)
