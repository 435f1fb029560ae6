"""CPU checks of the texture bake (no GPU): the numpy restatement of tests/texture_reference.py against what the reference's own
stages gave (tests/golden/ref_texture_pins.npz, written by tests/golden/make_texture_golden.py), the atlas' properties, the
orbit poses, the restated rasterizer's coverage rules on the hand-made faces, and the OBJ + PNG writer.

The grid-put gate is the project's standing one (MARGIN / FLOOR of tests/test_gpu_mesh.py): max |x - x64| over the texels,
x64 the float64 restatement on the same input, must stay within 8 x the same error of the reference's own float32 result,
with a floor of 64 float32 ulps (64 * 2^-23, absolute)."""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import texture_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 8
FLOOR = 64 * 2.0 ** -23


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(HERE, "golden", "ref_texture_pins.npz"))


def gate(name, ours, theirs, truth):
    err, ref_err = np.abs(ours - truth).max(initial=0.0), np.abs(theirs - truth).max(initial=0.0)
    print(f"{name}: {err:.3e} / {ref_err:.3e}, floor {FLOOR:.3e}, bit-equal {np.array_equal(ours, theirs)}")
    assert err <= max(MARGIN * ref_err, FLOOR)


# ---- grid put ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", ref.PUT_SIZES)
def test_grid_put_restatement_against_the_reference(pins, N):
    coords, values, valid = ref.put_case(N)
    H, W, mr = ref.PUT_H, ref.PUT_W, ref.PUT_MIN_RESOLUTION
    assert ref.levels(H, W, mr) == [(64, 64), (32, 32)]
    res, cnt = ref.grid_put(H, W, coords, values, valid, mr)
    res64, cnt64 = ref.grid_put(H, W, coords, values, valid, mr, dtype=np.float64)
    assert res.dtype == np.float32 and cnt.dtype == np.float32
    gate(f"put{N} result", res, pins[f"put{N}_result"], res64)
    gate(f"put{N} count", cnt, pins[f"put{N}_count"], cnt64)
    assert np.array_equal(cnt == 0, pins[f"put{N}_count"] == 0) and np.array_equal(cnt == 0, cnt64 == 0)
    for size in (64, 32):
        r, c = ref.linear_put(size, size, coords, values, valid)
        r64, c64 = ref.linear_put(size, size, coords, values, valid, dtype=np.float64)
        gate(f"lin{N}_{size} result", r, pins[f"lin{N}_{size}_result"], r64)
        gate(f"lin{N}_{size} count", c, pins[f"lin{N}_{size}_count"], c64)
        assert np.array_equal(c == 0, pins[f"lin{N}_{size}_count"] == 0)


def test_grid_put_case_has_what_it_promises():
    coords, values, valid = ref.put_case(5000)
    assert {(-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0)} <= {tuple(c) for c in coords[:8].tolist()}
    assert abs(int((~valid).sum()) - 5000 // 3) <= 8
    i = np.floor((coords[1000:3000] * 0.5 + 0.5) * 63)
    assert len(np.unique(i, axis=0)) == 1  # 2000 samples with one base texel
    _, cnt = ref.linear_put(64, 64, coords, values, valid)
    assert cnt.max() > 300  # ... so its four texels hold long runs (two thirds of 2000 split over four taps)


def test_accumulate_first_view_wins():
    views = ref.views_case()
    albedo, cnt = np.zeros((32, 32, 3), np.float32), np.zeros((32, 32), np.float32)
    history = []
    for cur, cc in views:
        before = cnt.copy()
        albedo, cnt = ref.accumulate(albedo, cnt, cur, cc)
        history.append((before, cnt.copy()))
    before, after = history[1]
    won = before >= np.float32(0.1)
    assert won.any() and (views[1][1][won] > 0).any()  # the second view would overwrite these but for the rule
    assert np.array_equal(after[won], before[won])
    out, mask = ref.normalize(albedo, cnt)
    assert np.array_equal(mask, cnt > 0) and np.all(np.isfinite(out))


# ---- fill -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.fill_masks()))
def test_fill_restatement_against_scipy_and_sklearn(pins, name):
    mask = ref.fill_masks()[name]
    near, d2 = ref.fill_nearest(mask, ref.FILL_RADIUS)
    check_fill(pins, name, near, d2)
    albedo = ref.fill_albedo()
    out, _ = ref.fill(albedo, mask, ref.FILL_RADIUS)
    assert np.array_equal(out[mask], albedo[mask]) and np.array_equal(out[near < 0], albedo[near < 0])


def check_fill(pins, name, near, d2):
    """near int32 [h, w] (-1 outside the inpaint region), d2 [h, w] or None (then derived from near) against the pins: the
    region equal, the squared distance equal for every inpaint texel, the index equal wherever the nearest is unique; at most
    10 % of the inpaint texels may be left out of the index comparison."""
    w = near.shape[1]
    assert np.array_equal(near >= 0, pins[f"fill_{name}_region"])
    at = pins[f"fill_{name}_inpaint"].astype(np.int64)
    assert np.array_equal(np.stack(np.nonzero(near >= 0), axis=-1), at)
    got = near[at[:, 0], at[:, 1]].astype(np.int64)
    rows, cols = got // w, got % w
    got_d2 = (rows - at[:, 0]) ** 2 + (cols - at[:, 1]) ** 2
    assert np.array_equal(got_d2, pins[f"fill_{name}_d2"])
    if d2 is not None:
        assert np.array_equal(d2[at[:, 0], at[:, 1]], pins[f"fill_{name}_d2"])
    ties = pins[f"fill_{name}_ties"]
    share = float(ties.mean()) if len(ties) else 0.0
    print(f"fill {name}: {len(at)} inpaint texels, {100 * share:.1f} % with more than one nearest")
    assert share <= 0.10
    want = pins[f"fill_{name}_nearest"].astype(np.int64)
    assert np.array_equal(np.stack([rows, cols], axis=1)[~ties], want[~ties])


# ---- cameras ----------------------------------------------------------------------------------------------------------------
def test_orbit_poses_against_the_reference(pins):
    from goi_hyperplane_amd import texture
    cams = texture.orbit_cameras(64, radius=2)
    got = np.stack([c.pose for c in cams])
    want = pins["orbit_poses"]
    assert got.shape == want.shape == (26, 4, 4) and got.dtype == np.float32
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    assert np.all(np.abs(got - want) <= ulp)
    for c in cams:  # the camera sees the origin: it lies on the axis, in front, at the orbit's distance
        o = np.array([0, 0, 0, 1], np.float32) @ c.full_proj_transform
        assert o[3] > 0 and abs(o[3] - 2) < 1e-5 and abs(o[0] / o[3]) < 1e-5 and abs(o[1] / o[3]) < 1e-5
        assert np.allclose(c.camera_center, c.pose[:3, 3]) and (c.image_width, c.image_height) == (64, 64)
    legacy = texture.orbit_cameras(64, radius=2, rectify=False)[3]  # the reference's MiniCam as it stands
    assert np.array_equal(legacy.world_view_transform, np.linalg.inv(legacy.pose).T)
    assert np.array_equal(legacy.camera_center, -legacy.pose[:3, 3])


# ---- atlas ------------------------------------------------------------------------------------------------------------------
def _point_segment(p, a, b):
    ab, ap = b - a, p - a
    t = np.clip((ap * ab).sum(-1) / (ab * ab).sum(-1), 0, 1)
    return np.linalg.norm(ap - t[..., None] * ab, axis=-1)


def triangle_distance(A, B):
    """The distance of disjoint triangles A, B [..., 3, 2]: the smallest corner-to-edge distance, both ways."""
    d = np.full(A.shape[:-2], np.inf)
    for P, Q in ((A, B), (B, A)):
        for i in range(3):
            for j in range(3):
                d = np.minimum(d, _point_segment(P[..., i, :], Q[..., j, :], Q[..., (j + 1) % 3, :]))
    return d


def texels_inside(tri, y, x):
    """texel centres (y, x) inside or on the triangle tri [..., 3, 2] of (x, y) corners (positive area)"""
    inside = True
    for k in range(3):
        a, b = tri[..., k, :], tri[..., (k + 1) % 3, :]
        inside = inside & ((b[..., 0] - a[..., 0]) * (y - a[..., 1]) - (b[..., 1] - a[..., 1]) * (x - a[..., 0]) >= -1e-9)
    return inside


@pytest.mark.parametrize("size", [64, 256])
@pytest.mark.parametrize("F", [0, 1, 2, 3, 7, 5000])
def test_atlas_properties(F, size):
    from goi_hyperplane_amd import texture
    if F == 5000 and size == 64:
        with pytest.raises(ValueError, match="at least 4"):
            texture.atlas(F, size)
        return
    faces = torch.from_numpy(np.random.default_rng(F).integers(0, max(F, 1), size=(F, 3)).astype(np.int32))
    at = texture.atlas(F, size, faces=faces)
    again = texture.atlas(F, size)
    assert torch.equal(at.vt, again.vt) and torch.equal(at.ft, again.ft) and again.vmapping is None  # a function of (F, size)
    assert at.ft.dtype == torch.int32 and torch.equal(at.ft, torch.arange(3 * F, dtype=torch.int32).view(F, 3))
    assert torch.equal(at.vmapping, faces.view(-1))
    want_vt, _, _, (n, cell) = ref.atlas(F, size)
    vt = at.vt.numpy()
    assert vt.dtype == np.float32 and vt.shape == (3 * F, 2) and np.array_equal(vt.view(np.int32), want_vt.view(np.int32))
    assert cell >= 4 and n * cell <= size
    if F == 0:
        return
    tri = vt.astype(np.float64).reshape(F, 3, 2) * (size - 1)  # texel units; x = u (columns), y = v (rows)
    d1, d2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    assert np.all(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0] > 0.4)  # positive area (at least a one-texel leg)
    p = np.arange(F) // 2
    origin = np.stack([cell * (p % n), cell * (p // n)], axis=1)[:, None, :]
    eps = 1e-3  # float32 vt: 256 * 2^-24 texels
    assert np.all(tri >= origin + 0.5 - eps) and np.all(tri <= origin + cell - 1.5 + eps)  # inside its own cell, half a texel in:
    #                                                          triangles of different cells are at least two texels apart
    if F > 1:  # the two triangles of a cell: at least one texel apart
        m = F // 2
        assert np.all(triangle_distance(tri[0:2 * m:2], tri[1:2 * m:2]) >= 1 - eps)
    # no texel centre inside two triangles: count, per texel, the triangles it lies in (a triangle stays in its cell, so its
    # cell's texels are the only candidates)
    yy, xx = np.meshgrid(np.arange(cell), np.arange(cell), indexing="ij")
    y, x = origin[:, :, 1, None] + yy[None], origin[:, :, 0, None] + xx[None]  # [F, cell, cell]
    inside = texels_inside(tri[:, None, None], y, x)
    assert np.all(inside.reshape(F, -1).sum(axis=1) >= 1)  # and every triangle holds a texel centre
    hits = np.zeros((size, size), np.int64)
    np.add.at(hits, (y[inside], x[inside]), 1)
    assert hits.max() == 1


# ---- rasterizer rules on the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (45, 67)])
def test_restated_rasterizer_rules(H, W):
    cases = ref.hand_cases(H, W)
    check_hand_cases(H, W, {k: ref.rasterize(v, f, H, W) for k, (v, f) in cases.items()})
    info = {}
    ref.rasterize(*cases["all"], H, W, info)
    assert info["large"] and len(info["large"]) < len(cases["all"][1]) - 3  # both paths of pass 1 have work
    info = {}
    ref.rasterize(*cases["shared_edge"], H, W, info)
    assert info["covered"].sum() == 36 * 36  # every pixel of the quad exactly once, the diagonal included


def check_hand_cases(H, W, out):
    """out: name -> (tri, bary, zw) as numpy arrays"""
    tri = {k: np.asarray(v[0]) for k, v in out.items()}
    t = tri["shared_edge"]
    assert (t > 0).sum() == 36 * 36 and np.all(t[np.arange(5, 40), np.arange(5, 40)] == 2)  # the diagonal: face 1's alone
    assert set(np.unique(tri["coplanar"])) == {0, 1}  # equal depth bits: the lower face
    assert np.all(tri["full_frame"] == 1)
    assert not tri["sliver"].any() and not tri["zero_area"].any()
    assert 0 < (tri["half_off"] > 0).sum() and tri["half_off"][:, 0].any()
    assert set(np.unique(tri["w_nonpositive"])) == {0, 1}
    assert (tri["back_facing"] > 0).sum() > 300
    assert not tri["no_faces"].any() and not np.asarray(out["no_faces"][1]).any() and not np.asarray(out["no_faces"][2]).any()
    for k, (t, bary, zw) in out.items():
        t, bary, zw = np.asarray(t), np.asarray(bary), np.asarray(zw)
        assert t.shape == (H, W) and bary.shape == (H, W, 2) and zw.shape == (H, W)
        assert not bary[t == 0].any() and not zw[t == 0].any()
        b = bary[t > 0]
        assert np.all(b >= 0) and np.all(b.sum(axis=1) <= 1 + 1e-6)


# ---- OBJ + PNG --------------------------------------------------------------------------------------------------------------
def decode_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()  # filter 0 on every row
    return raw[:, 1:].reshape(h, w, 3)


def test_obj_and_png_round_trip(tmp_path):
    from goi_hyperplane_amd import io, texture
    rng = np.random.default_rng(5)
    F = 7
    at = texture.atlas(F, 64)
    v = torch.from_numpy(rng.normal(size=(3 * F, 3)).astype(np.float32))
    n = torch.from_numpy(rng.normal(size=(3 * F, 3)).astype(np.float32))
    albedo = torch.from_numpy(rng.uniform(0, 1, size=(64, 48, 3)).astype(np.float32))
    albedo[0, 0] = torch.tensor([0.0, 1.0, 0.5])
    m = texture.TexturedMesh(v, at.ft, at.vt, at.ft, n, albedo, torch.ones(64, 48, dtype=torch.bool))
    path = str(tmp_path / "sub" / "mesh.obj")
    io.save_mesh_obj(path, m)
    back = io.read_mesh_obj(path)
    assert np.array_equal(back["faces"], at.ft.numpy()) and np.array_equal(back["ft"], at.ft.numpy())
    assert np.array_equal(back["fn"], at.ft.numpy()) and back["faces"].dtype == np.int32
    assert np.array_equal(back["vertices"], v.numpy()) and np.array_equal(back["normals"], n.numpy())  # equal as printed
    vt = at.vt.numpy()
    assert np.array_equal(back["vt"][:, 0], vt[:, 0]) and np.array_equal(back["vt"][:, 1], np.float32(1) - vt[:, 1])
    assert back["mtllib"] == "mesh.mtl" and back["usemtl"] == "defaultMat"
    assert back["mtl"] == {"newmtl": "defaultMat", "Ka": "1 1 1", "Kd": "1 1 1", "Ks": "0 0 0", "Tr": "1", "illum": "1", "Ns": "0",
                           "map_Kd": "mesh_albedo.png"}
    first = open(path).readline()
    assert first == "mtllib mesh.mtl \n"
    png = decode_png(str(tmp_path / "sub" / "mesh_albedo.png"))
    assert np.array_equal(png, (albedo.numpy() * 255).astype(np.uint8)) and tuple(png[0, 0]) == (0, 255, 127)
    with pytest.raises(ValueError):
        io.save_mesh_obj(str(tmp_path / "mesh.ply"), m)


def test_no_cpu_fallback():
    from goi_hyperplane_amd import texture
    v, f = ref.hand_cases(64, 64)["coplanar"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.rasterize(torch.from_numpy(v), torch.from_numpy(f), 64, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.fill(torch.zeros(8, 8, 3), torch.zeros(8, 8, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        texture.grid_put(64, 64, torch.zeros(4, 2), torch.zeros(4, 3))
