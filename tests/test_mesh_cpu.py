"""The numpy restatements of tests/mesh_reference.py checked on their own (no GPU): components against scipy, the pinned counts
of the test meshes, the bisection's invariant, the normals against the reference's own auto_normal
(tests/golden/ref_mesh_pins.npz), and the PLY normals."""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import field_reference as fref
from tests import mesh_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))


def scipy_labels(f, V):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(f, dtype=np.int64)
    i, j = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    _, lab = connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(V, V)), directed=False)
    first = np.full(lab.max() + 1, V, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(V))
    named = np.zeros(V, dtype=bool)
    named[f.reshape(-1)] = True
    return np.where(named, first[lab], -1).astype(np.int32)


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "equal", "blobs", "noisy24"])
def test_components_match_scipy(name):
    v, f, _ = ref.grid_mesh(name)
    vl, fl = ref.components(f, len(v))
    assert np.array_equal(vl, scipy_labels(f, len(v))) and np.array_equal(fl, vl[f[:, 0]])


def test_components_of_the_permuted_strip():
    v, f = ref.permuted_strip()
    vl, _ = ref.components(f, len(v))
    assert len(f) == 4096 and np.array_equal(vl, scipy_labels(f, len(v))) and np.all(vl == 0)


def test_blobs_counts():
    v, f, c = ref.grid_mesh("blobs")
    assert (len(v), len(f)) == (15946, 31558)
    info = {}
    ref.clean(v, f, c, 64, 0.2, info)
    assert len(info["roots"]) == 28 and (info["faces"].min(), info["faces"].max()) == (68, 4820)
    assert round(float(info["diag"].min()), 3) == 0.044 and round(float(info["diag"].max()), 3) == 0.436
    assert int(info["keep"].sum()) == 8 and info["nulls_and_duplicates"] == 0
    ref.clean(v, f, c, 200, 0.1, info)
    small, short = info["faces"] < 200, info["diag"] < 0.1
    assert int(info["keep"].sum()) == 18 and int((short & ~small).sum()) == 6 and int((small & ~short).sum()) == 0
    assert len(ref.clean(v, f, c, 0, 0)[1]) == len(f)


def test_noisy24_counts():
    v, f, _ = ref.grid_mesh("noisy24")
    vl, fl = ref.components(f, len(v))
    sizes = np.sort(np.bincount(fl, minlength=len(v))[np.unique(vl[vl >= 0])])
    assert (len(v), len(f)) == (45142, 91754) and sizes.tolist() == [2, 4, 4, 4, 4, 12, 12, 12, 12, 24, 91664]
    assert ref.cancellation(v, f).min() > 0.02


def test_dirty_blobs():
    v, f, c = ref.dirty_blobs()
    bv, bf, _ = ref.grid_mesh("blobs")
    info = {}
    out = ref.clean(v, f, c, 64, 0.2, info)
    assert len(f) == len(bf) + 20 + 3 and info["nulls_and_duplicates"] == 3
    small, short = info["faces"] < 64, info["diag"] < 0.2
    assert int((small & ~short).sum()) == 1  # the strip: removed by the face count alone
    clean_blobs = ref.clean(bv, bf, None, 64, 0.2)
    assert np.array_equal(out[0], clean_blobs[0]) and np.array_equal(out[1], clean_blobs[1])
    assert np.array_equal(v[out[3]], out[0]) and np.array_equal(c[out[3]], out[2])
    assert len(ref.clean(v, f, c, 10 ** 9, 0)[1]) == 0


def test_clean_removes_the_zero_area_faces_of_equal_grid():
    v, f, c = ref.grid_mesh("equal")
    info = {}
    out = ref.clean(v, f, c, 0, 0, info)
    assert len(f) == 360 and info["nulls_and_duplicates"] == 216 and len(out[1]) == 144
    n = ref.cross_f32(out[0], out[1])
    assert np.all(np.abs(n).sum(axis=1) > 0)


@pytest.mark.parametrize("divisions,cells,distinct,faces", [(6, 118, 202, 181), (12, 494, 955, 900), (24, 1807, 3574, 3490)])
def test_clustering_counts_on_blobs(divisions, cells, distinct, faces):
    v, f, c = ref.grid_mesh("blobs")
    info = {}
    out = ref.decimate(v, f, c, divisions=divisions, info=info)
    assert (info["cells"], info["distinct"], len(out[1])) == (cells, distinct, faces)
    assert info["distinct"] == ref.probe_count(v, f, divisions)
    assert out[1].max() == len(out[0]) - 1 and np.all(np.diff(info["keys"]) > 0)
    used = out[4] >= 0
    # the mean of the members of every output vertex, in float64 and in any order, agrees to rounding
    mean = np.stack([np.bincount(out[4][used], weights=v[used, k].astype(np.float64)) for k in range(3)], axis=1)
    mean /= np.bincount(out[4][used])[:, None]
    assert np.allclose(out[0], mean, rtol=1e-6, atol=1e-6)


def test_clustering_is_not_manifold_preserving():
    v, f, _ = ref.grid_mesh("torus")
    out = ref.decimate(v, f, None, divisions=16)
    assert max(fref.mesh_topology(out[1], len(out[0]))["edge_use"]) > 2  # edges used 3 times: welded sheets


def test_bisection_invariant():
    v, f, c = ref.grid_mesh("sphere48")
    assert len(f) == 41536
    for target in (2000, 300, 5):
        calls = []

        def count(n):
            calls.append(n)
            return ref.probe_count(v, f, n)
        n = ref.bisect_divisions(count, target)
        assert len(calls) <= 11 and (n == 1 or ref.probe_count(v, f, n) <= target)
        out = ref.decimate(v, f, c, target_faces=target)
        assert out[3] == n and len(out[1]) <= target
    assert ref.decimate(v, f, c, target_faces=2000)[3] == 15
    same = ref.decimate(v, f, c, target_faces=len(f))
    assert same[3] == 0 and np.array_equal(same[1], f) and np.array_equal(same[4], np.arange(len(v)))


def test_package_bisection_is_the_restatement():
    from goi_hyperplane_amd import mesh
    table = {n: (n * n * 7) % 5000 + n for n in range(1, 1025)}  # not monotone
    for target in (0, 10, 999, 4000, 10 ** 7):
        assert mesh.bisect_divisions(table.__getitem__, target) == ref.bisect_divisions(table.__getitem__, target)


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "equal"])
def test_normals_restatement_against_the_reference_pin(name):
    pins = np.load(os.path.join(HERE, "golden", "ref_mesh_pins.npz"))
    v, f, _ = ref.grid_mesh(name)
    assert np.array_equal(pins[name + "_v"], v) and np.array_equal(pins[name + "_f"], f)
    theirs, truth = pins[name + "_vn"], ref.vertex_normals(v, f, dtype=np.float64)
    assert ref.cancellation(v, f).min() >= 1e-3
    ref_err = np.abs(theirs - truth).max()
    for order in ("face", "corner"):
        err = np.abs(ref.vertex_normals(v, f, order=order) - truth).max()
        assert err <= max(8 * ref_err, 64 * 2.0 ** -23)
        assert np.abs(ref.vertex_normals(v, f, order=order) - theirs).max() <= 8 * 2.0 ** -23  # (torch's cross contracts)


def test_save_mesh_ply_without_normals_is_unchanged(tmp_path):
    from goi_hyperplane_amd import io
    v, f, c = ref.grid_mesh("sphere")
    col = np.clip(c, 0, 1)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    io.save_mesh_ply(a, v, f, col)
    # the writer as it stood before normals existed: header and records spelled out
    vrec = np.empty(len(v), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    c8 = np.rint(col.astype(np.float64) * 255.0).astype(np.uint8)
    vrec["red"], vrec["green"], vrec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"], frec["i"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
              "property list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
    with open(b, "wb") as fh:
        fh.write(header.encode("ascii") + vrec.tobytes() + frec.tobytes())
    assert open(a, "rb").read() == open(b, "rb").read()
    assert len(io.read_mesh_ply(a)) == 3 and io.read_mesh_ply(a, with_normals=True)[3] is None


def test_ply_normals_round_trip(tmp_path):
    from goi_hyperplane_amd import io
    v, f, c = ref.grid_mesh("torus")
    n = ref.vertex_normals(v, f)
    for col in (None, np.clip(c, 0, 1)):
        path = str(tmp_path / "n.ply")
        io.save_mesh_ply(path, v, f, col, normals=n)
        head = open(path, "rb").read(400).decode("ascii", "replace")
        assert head.index("property float z") < head.index("property float nx") < head.index("property float nz")
        assert col is None or head.index("property float nz") < head.index("property uchar red")
        rv, rf, rc, rn = io.read_mesh_ply(path, with_normals=True)
        assert np.array_equal(rv, v) and np.array_equal(rf, f) and np.array_equal(rn.view(np.int32), n.view(np.int32))
        assert (rc is None) == (col is None) and len(io.read_mesh_ply(path)) == 3
    with pytest.raises(ValueError):
        io.save_mesh_ply(path, v, f, normals=n[:-1])


def test_lib_declares_every_mesh_symbol():
    import re
    from goi_hyperplane_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "goi_raster.h")).read()
    declared = set(re.findall(r"^(?:int|size_t) (goi_mesh_\w+)\(", header, flags=re.M))
    assert len(declared) == 12 and declared == set(_lib.MESH_SYMBOLS)
    for name in declared:  # and under ABI 8's later additions
        assert name in header[:header.index("#define GOI_RASTER_ABI_VERSION")]
    assert _lib.ABI_VERSION == 9  # (9 changed the frame entries; the mesh family is as 8 added it)


def test_mesh_module_validates_before_it_needs_a_gpu():
    import torch
    from goi_hyperplane_amd import mesh
    v, f = torch.zeros(4, 3), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.components(f, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.vertex_normals(v, f)
    for bad in (lambda: mesh.components(f.long(), 4), lambda: mesh.components(f, -1), lambda: mesh.clean(v.double(), f),
                lambda: mesh.clean(v, f, min_faces=-1), lambda: mesh.clean(v, f, torch.zeros(3, 3)),
                lambda: mesh.decimate(v, f), lambda: mesh.vertex_normals(v[:, :2], f)):
        with pytest.raises(ValueError):
            bad()
