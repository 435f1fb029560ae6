"""goi_hyperplane_amd.texture (csrc/texture.hip) on the GPU: rasterize, resolve, grid_put, accumulate / normalize, fill, the
pixel alignment with the Gaussian rasterizer, and bake end to end.

Every function is compared with its numpy restatement (tests/texture_reference.py): integers equal, floats bit for bit (the
device's float32 division and sqrt are IEEE and the unit is compiled without contraction, so no ulp allowance is used), and
every call is made twice and must give the same bits.  grid_put is also held against the reference's own results
(tests/golden/ref_texture_pins.npz) with the gate of tests/test_texture_cpu.py, fill against scipy's regions and sklearn's
distances.  The inputs (samples, masks, hand-made faces) are tests/texture_reference.py's, shared with the CPU tests."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import field_reference as fref
from tests import texture_reference as ref
from tests.test_texture_cpu import check_fill, check_hand_cases, gate, pins, texels_inside  # noqa: F401  (pins: a fixture)

pytestmark = pytest.mark.gpu

MASKS = ref.fill_masks()  # disc, two, border, boxes, single, empty, full: defined once, for the pins' maker as well


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def T():
    from goi_hyperplane_amd import texture
    return texture


def up(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and np.array_equal(bits(a), bits(b))


def same_twice(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def check_raster(dev, v_clip, faces, H, W):
    want = ref.rasterize(v_clip, faces, H, W)
    v, f = up(v_clip, dev), up(faces, dev)
    got, again = T().rasterize(v, f, H, W), T().rasterize(v, f, H, W)
    assert int(got.status) == 0
    assert got.tri.dtype == torch.int32 and np.array_equal(got.tri.cpu().numpy(), want[0])
    assert same_bits(got.bary, want[1]) and same_bits(got.zw, want[2])
    assert same_twice(got[:3], again[:3])
    return got


# ---- rasterize --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (45, 67)])
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_rasterize_iso_surfaces(dev, name, H, W):
    v, f, _ = ref.unit_mesh(name)
    hit = 0
    for view in (0, 9, 24):  # level, from below at 45 degrees, straight down
        cam = T().orbit_cameras(64)[view]
        got = check_raster(dev, ref.clip_positions(v, cam.full_proj_transform), f, H, W)
        hit += int((got.tri > 0).sum())
    assert hit > 1500


@pytest.mark.parametrize("H,W", [(64, 64), (45, 67)])
def test_rasterize_hand_made_faces(dev, H, W):
    """A shared edge (every pixel once), coplanar copies (the lower face), a whole-frame face (the second path of pass 1), a
    sliver, a face half off the screen, a w <= 0, no area, a back face, no faces at all, and all of them in one mesh."""
    out = {}
    for name, (v, f) in ref.hand_cases(H, W).items():
        got = check_raster(dev, v, f, H, W)
        out[name] = tuple(t.cpu().numpy() for t in got[:3])
    check_hand_cases(H, W, out)
    info = {}
    ref.rasterize(*ref.hand_cases(H, W)["all"], H, W, info)
    assert 0 < len(info["large"]) and (info["covered"][[i for i in range(12) if i not in info["large"]]] > 0).any()


def test_rasterize_flags_an_index_out_of_range(dev):
    v, _ = ref.hand_cases(64, 64)["coplanar"]
    f = np.array([[0, 1, 2], [3, 4, 99], [3, -1, 5]], np.int32)
    got = T().rasterize(up(v, dev), up(f, dev), 64, 64)
    assert int(got.status) == T().STATUS_RANGE and set(got.tri.unique().tolist()) == {0, 1}
    with pytest.raises(ValueError):
        T().check_status(got.status)


# ---- resolve ----------------------------------------------------------------------------------------------------------------
def test_resolve(dev):
    v, f, n = ref.unit_mesh("sphere")
    F = len(f)
    vt, ft, _, _ = ref.atlas(F, 256)
    vt = (vt * np.float32(1.3) - np.float32(0.1)).astype(np.float32)  # some uv leave [0, 1]: the clamp has work
    cam = T().orbit_cameras(64)[11]
    rot = np.ascontiguousarray(cam.pose[:3, :3])
    image = np.random.default_rng(2).uniform(0, 1, size=(3, 64, 64)).astype(np.float32)
    tri, bary, zw = ref.rasterize(ref.clip_positions(v, cam.full_proj_transform), f, 64, 64)
    info = {}
    want = ref.resolve(tri, bary, vt, ft, n, f, rot, image, info)
    cos, uv = info["viewcos"][tri.reshape(-1) > 0], info["uv"][tri.reshape(-1) > 0]
    assert (cos > 0.5).sum() > 100 and (cos <= 0.5).sum() > 30  # pixels on both sides of the view-cosine test
    assert (uv > 1).any() and (uv < 0).any() and want[0].min() == -1 and want[0].max() == 1
    r = T().rasterize(up(ref.clip_positions(v, cam.full_proj_transform), dev), up(f, dev), 64, 64)
    args = (r, up(vt, dev), up(ft, dev), up(n, dev), up(f, dev), up(rot, dev), up(image, dev))
    got, again = T().resolve(*args, return_status=True), T().resolve(*args)
    assert int(got[3]) == 0 and got[2].dtype == torch.bool
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and np.array_equal(got[2].cpu().numpy(), want[2])
    assert same_twice(got[:3], again)
    empty = want[2].reshape(64, 64)[tri == 0]
    assert not empty.any() and not got[0].cpu().numpy().reshape(64, 64, 2)[tri == 0].any()  # invalid pixels stay in place


# ---- grid put ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ref.PUT_SIZES)
def test_grid_put(dev, pins, N):  # noqa: F811
    coords, values, valid = ref.put_case(N)
    H, W, mr = ref.PUT_H, ref.PUT_W, ref.PUT_MIN_RESOLUTION
    want = ref.grid_put(H, W, coords, values, valid, mr)
    truth = ref.grid_put(H, W, coords, values, valid, mr, dtype=np.float64)
    args = (H, W, up(coords, dev), up(values, dev), up(valid, dev), mr)
    got, again = T().grid_put(*args, return_count=True, return_status=True), T().grid_put(*args, return_count=True)
    assert int(got[2]) == 0 and tuple(got[1].shape) == (H, W, 1)
    assert same_bits(got[0], want[0]) and same_bits(got[1][..., 0], want[1])
    assert same_twice(got[:2], again)
    res, cnt = got[0].cpu().numpy(), got[1][..., 0].cpu().numpy()
    gate(f"device put{N} result", res, pins[f"put{N}_result"], truth[0])
    gate(f"device put{N} count", cnt, pins[f"put{N}_count"], truth[1])
    assert np.array_equal(cnt == 0, pins[f"put{N}_count"] == 0)
    # the samples compacted by hand, no mask: the same texture; and the divided form
    keep = up(valid, dev)
    packed = T().grid_put(H, W, up(coords, dev)[keep], up(values, dev)[keep], None, mr, return_count=True)
    assert same_twice(got[:2], packed)
    divided = T().grid_put(*args)
    assert same_bits(divided, ref.normalize(*want)[0])


def test_grid_put_without_a_level(dev):
    coords, values, valid = ref.put_case(5000)
    got = T().grid_put(16, 16, up(coords, dev), up(values, dev), None, 16, return_count=True)  # min(level) > 16 never holds
    assert not got[0].any() and not got[1].any()


def test_accumulate_and_normalize(dev):
    """Three synthetic views; the second would overwrite texels the first has won but for the cnt < 0.1 rule."""
    views = ref.views_case()
    want_a, want_c = np.zeros((32, 32, 3), np.float32), np.zeros((32, 32), np.float32)
    runs = []
    for _ in range(2):
        albedo = torch.zeros((32, 32, 3), device=dev)
        cnt = torch.zeros((32, 32, 1), device=dev)
        for cur, cc in views:
            T().accumulate(albedo, cnt, up(cur, dev), up(cc, dev))
        runs.append((albedo, cnt) + T().normalize(albedo, cnt))
    for cur, cc in views:
        want_a, want_c = ref.accumulate(want_a, want_c, cur, cc)
    want_n, want_m = ref.normalize(want_a, want_c)
    albedo, cnt, out, mask = runs[0]
    assert same_bits(albedo, want_a) and same_bits(cnt[..., 0], want_c)
    assert same_bits(out, want_n) and mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want_m)
    assert same_twice(runs[0], runs[1])
    first_c = views[0][1]
    won = first_c >= np.float32(0.1)
    assert (views[1][1][won] > 0).any() and np.array_equal(cnt[..., 0].cpu().numpy()[won], first_c[won])


# ---- fill -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MASKS))
def test_fill(dev, pins, name):  # noqa: F811
    mask, albedo = MASKS[name], ref.fill_albedo()
    want, want_near = ref.fill(albedo, mask, ref.FILL_RADIUS)
    a, m = up(albedo, dev), up(mask, dev)
    got, again = T().fill(a, m, ref.FILL_RADIUS, return_index=True), T().fill(a, m, ref.FILL_RADIUS, return_index=True)
    assert same_twice(got, again) and same_bits(T().fill(a, m), want)
    near = got[1].cpu().numpy()
    assert near.dtype == np.int32 and np.array_equal(near, want_near)
    assert same_bits(got[0], want)
    check_fill(pins, name, near, None)


def test_fill_smaller_radius(dev):
    mask, albedo = MASKS["two"], ref.fill_albedo()
    for radius in (0, 5):
        got = T().fill(up(albedo, dev), up(mask, dev), radius, return_index=True)
        want, want_near = ref.fill(albedo, mask, radius)
        assert same_bits(got[0], want) and np.array_equal(got[1].cpu().numpy(), want_near)


# ---- the two rasterizers agree on where a point lands ----------------------------------------------------------------------
def gaussian_set(dev, xyz, rgb, scale, opacity, rotation=None):
    from goi_hyperplane_amd.render import GaussianSet
    P = len(xyz)
    shs = np.zeros((P, 16, 3), np.float32)
    shs[:, 0, :] = (np.asarray(rgb, np.float32) - 0.5) / 0.28209479177387814
    rot = np.tile(np.array([1, 0, 0, 0], np.float32), (P, 1)) if rotation is None else rotation
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    return GaussianSet(t(xyz), t(np.broadcast_to(scale, (P, 3))), t(rot), t(np.full((P, 1), opacity)), t(shs),
                       t(np.zeros((P, 16))))


def test_mesh_pixels_are_gaussian_pixels(dev):
    from goi_hyperplane_amd import render
    tri_v = np.array([[-0.5, -0.35, 0.1], [0.45, -0.2, -0.3], [0.17, 0.64, 0.41]], np.float32)
    centroid = tri_v.mean(axis=0, dtype=np.float64).astype(np.float32)
    pc = gaussian_set(dev, centroid[None], [[1.0, 1.0, 1.0]], 0.004, 0.99)
    for view in (0, 6, 14, 17):  # (views where the centroid is at least 0.07 pixels from a pixel boundary)
        cam = T().orbit_cameras(64)[view]
        c = ref.clip_positions(centroid[None], cam.full_proj_transform)[0]
        sx, sy = ((c[0] / c[3] + 1) * 64 - 1) / 2, ((c[1] / c[3] + 1) * 64 - 1) / 2
        assert min(abs(sx - np.floor(sx) - 0.5), abs(sy - np.floor(sy) - 0.5)) > 0.05, "the test wants a pixel that is not a toss-up"
        px, py = int(np.rint(sx)), int(np.rint(sy))
        image = render.render_gui(render.TorchCamera(cam, dev), pc, torch.zeros(3, device=dev))["image"]
        lum = image.detach().sum(dim=0)
        assert float(lum.max()) > 0.5
        assert divmod(int(lum.argmax()), 64) == (py, px)
        r = T().rasterize(up(ref.clip_positions(tri_v, cam.full_proj_transform), dev), up(np.array([[0, 1, 2]], np.int32), dev), 64, 64)
        assert int(r.tri[py, px]) == 1
        u, v = (float(x) for x in r.bary[py, px])
        assert max(abs(u - 1 / 3), abs(v - 1 / 3)) < 0.03  # the centroid's pixel carries the centroid's barycentrics


# ---- bake -------------------------------------------------------------------------------------------------------------------
def shell_scene(dev):
    """About 2000 Gaussians on a shell of radius 0.5 around the origin, sigma 0.1 (small enough that a rendered pixel shows
    the Gaussians next to it), red where x > 0 and blue elsewhere; and the density half-way up the shell's profile."""
    m = fref.sphere_shell_model(P=2000, radius=0.5, sigma=0.1)
    xyz = (m["xyz"] - m["shell_center"].astype(np.float32)).astype(np.float32)
    rgb = np.where(xyz[:, 0:1] > 0, np.array([[0.9, 0.1, 0.1]], np.float32), np.array([[0.1, 0.1, 0.9]], np.float32))
    rot = m["rotation"] / np.linalg.norm(m["rotation"], axis=1, keepdims=True)
    P = len(xyz)
    shs = np.zeros((P, 16, 3), np.float32)
    shs[:, 0, :] = (rgb - 0.5) / 0.28209479177387814
    from goi_hyperplane_amd.render import GaussianSet
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    pc = GaussianSet(t(xyz), t(m["scaling"]), t(rot), t(m["opacity"][:, None]), t(shs), t(np.zeros((P, 16))))
    return pc, 0.5 * m["thresh"]


def outer_sheet(geo):
    """The shell is hollow, so its iso-surface has an inner sheet no camera sees: keep the component of the farthest vertex."""
    from goi_hyperplane_amd import mesh
    comp = mesh.components(geo.faces, int(geo.vertices.shape[0]))
    assert int(comp.status) == 0
    far = int(geo.vertices.norm(dim=1).argmax())
    keep = comp.face_label == comp.vertex_label[far]
    return mesh.Mesh(geo.vertices, geo.faces[keep].contiguous(), geo.colors, geo.normals, geo.center, geo.scale)


def test_bake(dev, tmp_path):
    """bake end to end on the red / blue shell.  Two departures from taking mesh.extract's mesh as it comes, both forced by the
    scene: a shell of Gaussians small enough to render sharp colours is hollow, so its iso-surface has an inner sheet that no
    camera sees and whose texels could only be filled from neighbours of either colour -- outer_sheet keeps the component of
    the farthest vertex; and target_faces=2500 (about 1700 faces on the outer sheet) keeps the atlas' cells at the 4-texel
    minimum in a 128^2 texture.  (A solid shell, sigma = radius / 2, renders as one uniform mix of the two colours.)"""
    from goi_hyperplane_amd import io, mesh, render
    tx = T()
    pc, thresh = shell_scene(dev)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        geo = outer_sheet(mesh.extract(pc, density_thresh=thresh, resolution=32, num_blocks=2, relax_ratio=1.5, target_faces=2500))
    F = int(geo.faces.shape[0])
    assert 300 < F <= 2048  # (2048 faces: 32 x 32 cells of 4 texels at 128)
    radius = geo.vertices[geo.faces.long()].norm(dim=2)
    assert float(radius.min()) > 0.5 and float(radius.max()) < 0.8
    size, res = 128, 64
    out = tx.bake(pc, geo, bg, texture_size=size, render_resolution=res)
    again = tx.bake(pc, geo, bg, texture_size=size, render_resolution=res)
    assert same_twice(out, again)
    # the public pieces in order
    at = tx.atlas(F, size, faces=geo.faces)
    idx = at.vmapping.long()
    v, vn = geo.vertices[idx].contiguous(), geo.normals[idx].contiguous()
    albedo, cnt = torch.zeros((size, size, 3), device=dev), torch.zeros((size, size, 1), device=dev)
    cams = tx.orbit_cameras(res)
    assert len(cams) == 26
    with torch.no_grad():
        for cam in cams:
            tc = render.TorchCamera(cam, dev)
            image = render.render_gui(tc, pc, bg)["image"]
            r = tx.rasterize(tx.clip_positions(v, tc.full_proj_transform), at.ft, res, res)
            coords, values, valid = tx.resolve(r, at.vt, at.ft, vn, at.ft, up(np.ascontiguousarray(cam.pose[:3, :3]), dev), image)
            cur, cur_cnt = tx.grid_put(size, size, coords, values, valid, min_resolution=size // 4, return_count=True)
            tx.accumulate(albedo, cnt, cur, cur_cnt)
    normal, mask = tx.normalize(albedo, cnt)
    filled = tx.fill(normal, mask, 32)
    assert torch.equal(out.albedo, filled) and torch.equal(out.mask, mask)
    assert torch.equal(out.vertices, v) and torch.equal(out.normals, vn) and torch.equal(out.vt, at.vt)
    assert torch.equal(out.faces, at.ft) and torch.equal(out.ft, at.ft)
    a = out.albedo.cpu().numpy()
    assert a.shape == (size, size, 3) and np.all(np.isfinite(a)) and a.min() >= 0 and a.max() <= 1
    # every texel inside a UV triangle is textured: by a view, or by the fill
    _, _, texel, (n, cell) = ref.atlas(F, size)
    yy, xx = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    m = out.mask.cpu().numpy()
    near, _ = ref.fill_nearest(m, 32)
    textured = m | (near >= 0)
    centroid = geo.vertices[geo.faces.long()].mean(dim=1).cpu().numpy()
    red = blue = 0
    margin = 1.0
    for f in range(F):
        p = f // 2
        ys, xs = slice(cell * (p // n), cell * (p // n + 1)), slice(cell * (p % n), cell * (p % n + 1))
        inside = texels_inside(texel[f], yy[ys, xs], xx[ys, xs])
        assert inside.any() and textured[ys, xs][inside].all()
        mean = a[ys, xs][inside].mean(axis=0)
        if centroid[f, 0] > 0.2:
            assert mean[0] > mean[2], (f, centroid[f], mean)
            margin = min(margin, mean[0] - mean[2])
            red += 1
        elif centroid[f, 0] < -0.2:
            assert mean[2] > mean[0], (f, centroid[f], mean)
            margin = min(margin, mean[2] - mean[0])
            blue += 1
    assert red > F // 8 and blue > F // 8
    print(f"bake: F {F}, cell {cell}, {int(m.sum())} of {size * size} texels reached by a view, {red} red and {blue} blue faces, "
          f"smallest colour margin {margin:.3f}")
    path = str(tmp_path / "shell.obj")
    io.save_mesh_obj(path, out)
    back = io.read_mesh_obj(path)
    assert np.array_equal(back["vertices"], out.vertices.cpu().numpy()) and np.array_equal(back["faces"], out.faces.cpu().numpy())
    assert np.array_equal(back["normals"], out.normals.cpu().numpy()) and np.array_equal(back["ft"], out.ft.cpu().numpy())
    vt = out.vt.cpu().numpy()
    assert np.array_equal(back["vt"], np.stack([vt[:, 0], np.float32(1) - vt[:, 1]], axis=1))
    from tests.test_texture_cpu import decode_png
    assert np.array_equal(decode_png(str(tmp_path / "shell_albedo.png")), (a * 255).astype(np.uint8))
