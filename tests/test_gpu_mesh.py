"""goi_hyperplane_amd.mesh (csrc/mesh.hip) on the GPU: components, clean, decimate, vertex_normals and extract.

Every function is compared with its numpy restatement (tests/mesh_reference.py): integers equal, floats bit for bit.  The
device's float32 division and sqrt and its float64 -> float32 rounding are IEEE and the unit is compiled without contraction,
so no ulp allowance is used anywhere.  Meshes: the iso-surfaces of the analytic grids of tests/field_reference.py, `blobs`
(V 15 946, F 31 558, 28 components of 68 .. 4820 faces), blobs + a 20-triangle strip + dirt (a repeated index, two more copies
of a face in another rotation and orientation, a NaN vertex), noisy24 (V 45 142, F 91 754: one giant component and 10 of 2 .. 24
faces), a 4096-triangle strip numbered by a random permutation, sphere48 (F 41 536), the empty mesh and a single triangle.

Normals are also held against a float64 restatement: max |n - n64| over the vertices must stay within 8 x the error of the
reference's own float32 result on the same mesh (the pin of tests/golden/ref_mesh_pins.npz, or on the larger meshes the
restatement in the reference's (corner, face) order), floor 64 float32 ulps.  A vertex is left out only when its float64
|sum| / sum |contribution| is under 1e-3; none is on these meshes (smallest ratio 0.024 on noisy24, 0.21 on blobs).

Measured on an MI355X, max |n - n64| of the device / of the reference = ratio:
    sphere 2.09e-7 / 1.09e-7 = 1.92   torus 8.48e-7 / 9.24e-7 = 0.92   two_spheres 1.25e-7 / 1.11e-7 = 1.13
    equal 5.15e-8 / 5.15e-8 = 1.00   blobs 1.44e-6 / 1.44e-6 = 1.00   noisy24 6.09e-5 / 6.09e-5 = 1.00   strip 7.75e-8 / 7.75e-8 = 1.00
(no vertex left out on any mesh; on the larger meshes the vertex with the largest error is the same in both orders.)
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import field_reference as fref
from tests import mesh_reference as ref

pytestmark = pytest.mark.gpu

MARGIN = 8  # the gate of a float32 stage pinned to the reference
FLOOR = 64 * 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from goi_hyperplane_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def M():
    from goi_hyperplane_amd import mesh
    return mesh


def up(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)  # (a copy: the shared meshes are read-only)


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_ints(a, b):
    a = a.cpu().numpy()
    return a.dtype == np.int32 and a.shape == np.asarray(b).shape and np.array_equal(a, b)


def named_mesh(name):
    if name == "dirty_blobs":
        return ref.dirty_blobs()
    if name == "strip":
        return ref.permuted_strip() + (None,)
    if name == "empty":
        return np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32), None
    if name == "triangle":
        return np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[3, 0, 2]], np.int32), None
    return ref.grid_mesh(name)


# ---- components -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "equal", "blobs", "dirty_blobs", "noisy24", "strip", "empty",
                                  "triangle"])
def test_components(dev, name):
    v, f, _ = named_mesh(name)
    want_v, want_f = ref.components(f, len(v))
    faces = up(f, dev)
    got = M().components(faces, len(v))
    again = M().components(faces, len(v))
    assert int(got.status) == 0
    assert same_ints(got.vertex_label, want_v) and same_ints(got.face_label, want_f)
    assert torch.equal(got.vertex_label, again.vertex_label) and torch.equal(got.face_label, again.face_label)


def test_components_flags_an_index_out_of_range(dev):
    f = up(np.array([[0, 1, 2], [2, 3, 7], [4, 5, -1]], np.int32), dev)
    got = M().components(f, 6)
    assert int(got.status) == M().STATUS_RANGE
    assert got.vertex_label.tolist() == [0, 0, 0, -1, -1, -1] and got.face_label.tolist() == [0, 0, -1]
    with pytest.raises(ValueError):
        M().check_status(got.status)


# ---- clean ------------------------------------------------------------------------------------------------------------------
def check_clean(dev, v, f, c, min_faces, min_diag):
    want = ref.clean(v, f, c, min_faces, min_diag)
    got = M().clean(up(v, dev), up(f, dev), up(c, dev), min_faces, min_diag)
    print("clean", min_faces, min_diag, ": V", len(v), "->", tuple(got.vertices.shape), "F", len(f), "->", tuple(got.faces.shape))
    assert same_ints(got.faces, want[1]) and same_ints(got.vertex_index, want[3]) and same_ints(got.face_index, want[4])
    assert same_bits(got.vertices, want[0])
    assert (got.colors is None) == (c is None) and (c is None or same_bits(got.colors, want[2]))
    return got


@pytest.mark.parametrize("min_faces,min_diag", [(64, 0.2), (200, 0.1), (0, 0), (10 ** 9, 0)])
@pytest.mark.parametrize("name", ["dirty_blobs", "equal"])
def test_clean(dev, name, min_faces, min_diag):
    v, f, c = named_mesh(name)
    got = check_clean(dev, v, f, c, min_faces, min_diag)
    if min_faces == 10 ** 9:
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.colors.shape == (0, 3)


def test_clean_leaves_a_clean_sphere_alone(dev):
    v, f, c = named_mesh("sphere")
    got = check_clean(dev, v, f, None, 64, 0.2)
    assert same_bits(got.vertices, v) and same_ints(got.faces, f)
    assert same_ints(got.vertex_index, np.arange(len(v), dtype=np.int32)) and same_ints(got.face_index, np.arange(len(f), dtype=np.int32))


def test_clean_of_nothing(dev):
    v, f, _ = named_mesh("empty")
    got = M().clean(up(v, dev), up(f, dev))
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.colors is None and got.face_index.shape == (0,)


# ---- decimate ---------------------------------------------------------------------------------------------------------------
def check_decimate(dev, v, f, c, **kw):
    info = {}
    want = ref.decimate(v, f, c, info=info, **kw)
    got = M().decimate(up(v, dev), up(f, dev), up(c, dev), **kw)
    print("decimate", kw, ": divisions", got.divisions, "V", tuple(got.vertices.shape), "F", tuple(got.faces.shape))
    assert got.divisions == want[3]
    assert same_ints(got.faces, want[1]) and same_ints(got.cluster, want[4])
    assert same_bits(got.vertices, want[0])
    assert (got.colors is None) == (c is None) and (c is None or same_bits(got.colors, want[2]))
    return got, info


@pytest.mark.parametrize("divisions", [2, 6, 12, 24, 1024])
@pytest.mark.parametrize("name", ["blobs", "torus"])
def test_decimate(dev, name, divisions):
    v, f, c = named_mesh(name)
    got, info = check_decimate(dev, v, f, c, divisions=divisions)
    # every output vertex lies inside its cell's box (the mean of points of a box, rounded once)
    n, key = divisions, info["keys"]
    q = np.stack([key // (n * n), (key // n) % n, key % n], axis=1).astype(np.float64)
    out = got.vertices.cpu().numpy().astype(np.float64)
    lo, cell = info["lo"].astype(np.float64), float(info["cell"])
    slack = 4 * 2.0 ** -23 * np.abs(v).max()  # the float32 roundings of (v - lo) / cell and of the mean
    assert np.all(out >= lo + q * cell - slack)
    assert np.all((out <= lo + (q + 1) * cell + slack) | (q == n - 1))
    assert np.all(out <= v.max(axis=0) + slack)


def test_decimate_with_a_nan_vertex_and_dirt(dev):
    v, f, c = named_mesh("dirty_blobs")
    f = np.concatenate([f, np.array([[0, 1, len(v) - 1]], np.int32)])  # a face that names the NaN vertex
    check_decimate(dev, v, f, c, divisions=12)


def test_decimate_to_a_face_budget(dev):
    v, f, c = named_mesh("sphere48")
    assert len(f) == 41536
    got, _ = check_decimate(dev, v, f, c, target_faces=2000)
    assert 2 <= got.divisions <= 1024 and got.faces.shape[0] <= 2000
    assert ref.probe_count(v, f, got.divisions) <= 2000


@pytest.mark.parametrize("target", [41536, 10 ** 6])
def test_decimate_returns_a_mesh_within_budget_as_it_is(dev, target):
    v, f, c = named_mesh("sphere48")
    got, _ = check_decimate(dev, v, f, c, target_faces=target)
    assert got.divisions == 0 and same_bits(got.vertices, v) and same_ints(got.faces, f)


def test_decimate_arguments(dev):
    v, f, _ = named_mesh("sphere")
    tv, tf = up(v, dev), up(f, dev)
    for kw in (dict(), dict(divisions=4, target_faces=10), dict(divisions=1), dict(divisions=1025), dict(target_faces=-1)):
        with pytest.raises(ValueError):
            M().decimate(tv, tf, **kw)
    with pytest.raises(ValueError):
        M().decimate(tv, tf.long(), divisions=4)
    with pytest.raises(RuntimeError):
        M().decimate(tv.cpu(), tf.cpu(), divisions=4)


# ---- normals ----------------------------------------------------------------------------------------------------------------
PINNED = ("sphere", "torus", "two_spheres", "equal")


@pytest.mark.parametrize("name", list(PINNED) + ["blobs", "noisy24", "strip"])
def test_vertex_normals(dev, name):
    v, f, _ = named_mesh(name)
    got = M().vertex_normals(up(v, dev), up(f, dev)).cpu().numpy()
    assert same_bits(got, ref.vertex_normals(v, f))
    truth = ref.vertex_normals(v, f, dtype=np.float64)
    if name in PINNED:
        pins = np.load(fref.__file__.replace("field_reference.py", "golden/ref_mesh_pins.npz"))
        assert np.array_equal(pins[name + "_v"], v) and np.array_equal(pins[name + "_f"], f)
        theirs = pins[name + "_vn"]
    else:
        theirs = ref.vertex_normals(v, f, order="corner")
    take = ref.cancellation(v, f) >= 1e-3
    assert (~take).sum() <= 0.01 * len(v)
    err = np.abs(got[take] - truth[take]).max()
    ref_err = np.abs(theirs[take] - truth[take]).max()
    print(f"normals {name}: {err:.2e} / {ref_err:.2e} = {err / ref_err:.2f}, {int((~take).sum())} of {len(v)} left out")
    assert err <= max(MARGIN * ref_err, FLOOR)


def test_vertex_normals_default(dev):
    """An unreferenced vertex and a vertex whose faces cancel give (0, 0, 1)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 2, 2]], np.float32)
    f = np.array([[4, 1, 2], [4, 2, 1], [0, 1, 2]], np.int32)  # vertex 4: two opposite faces; vertex 3: none
    got = M().vertex_normals(up(v, dev), up(f, dev)).cpu().numpy()
    assert same_bits(got, ref.vertex_normals(v, f))
    assert got[3].tolist() == [0, 0, 1] and got[4].tolist() == [0, 0, 1] and got[0].tolist() == [0, 0, 1]
    empty = M().vertex_normals(up(v, dev), up(f[:0], dev)).cpu().numpy()
    assert np.array_equal(empty, np.tile(np.array([0, 0, 1], np.float32), (5, 1)))


# ---- no host synchronisation ------------------------------------------------------------------------------------------------
def count_syncs(fn):
    """Runs fn with torch's synchronisation warnings on and returns how many it raised."""
    import warnings
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    return sum("synchroniz" in str(w.message) for w in caught)


def test_components_and_normals_never_synchronise(dev):
    v, f, _ = named_mesh("torus")
    tv, tf = up(v, dev), up(f, dev)
    first = M().components(tf, len(v))  # loads the library and warms up outside the checked region
    n0 = M().vertex_normals(tv, tf)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        c = M().components(tf, len(v))
        n = M().vertex_normals(tv, tf)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(c.vertex_label, first.vertex_label) and torch.equal(n, n0)


def test_clean_and_decimate_synchronise_only_for_their_counts(dev):
    v, f, c = named_mesh("sphere48")
    tv, tf, tc = up(v, dev), up(f, dev), up(c, dev)
    M().clean(tv, tf, tc)
    M().decimate(tv, tf, tc, divisions=8)
    assert count_syncs(lambda: M().clean(tv, tf, tc)) == 1
    assert count_syncs(lambda: M().decimate(tv, tf, tc, divisions=8)) == 1
    probes = []
    ref.bisect_divisions(lambda n: probes.append(n) or ref.probe_count(v, f, n), 2000)
    assert count_syncs(lambda: M().decimate(tv, tf, tc, target_faces=2000)) == len(probes) + 1


# ---- end to end -------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, m, dev):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.get_xyz, self.get_opacity = t(m["xyz"]), t(m["opacity"])[:, None]
        self.get_scaling, self.get_rotation = t(m["scaling"]), t(m["rotation"])
        self.get_features = ((t(m["rgb"]) - 0.5) / 0.28209479177387814)[:, None, :]


def test_extract(dev, tmp_path):
    from goi_hyperplane_amd import io
    m = fref.sphere_shell_model()
    pc = Model(m, dev)
    kw = dict(density_thresh=m["thresh"], resolution=32, num_blocks=2, relax_ratio=1.5)
    raw = M().extract(pc, target_faces=None, normals=False, **kw)
    out = M().extract(pc, target_faces=500, **kw)
    F = int(out.faces.shape[0])
    print("extract: raw F", int(raw.faces.shape[0]), "-> F", F, "V", int(out.vertices.shape[0]))
    assert raw.normals is None and int(raw.faces.shape[0]) > 500 and 0 < F <= 500
    comp = M().components(out.faces, int(out.vertices.shape[0]))
    assert int(comp.status) == 0 and comp.vertex_label.unique().tolist() == [0]
    v, n = out.vertices.cpu().numpy().astype(np.float64), out.normals.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-5)
    assert np.all(((v - m["shell_center"]) * n).sum(axis=1) > 0)
    assert out.colors.shape == out.vertices.shape and float(out.colors.min()) >= 0 and float(out.colors.max()) <= 1
    path = str(tmp_path / "mesh.ply")
    io.save_mesh_ply(path, out.vertices, out.faces, out.colors, out.normals)
    rv, rf, rc, rn = io.read_mesh_ply(path, with_normals=True)
    assert same_bits(rv, out.vertices) and same_ints(out.faces, rf) and same_bits(rn, out.normals) and rc.shape == rv.shape
