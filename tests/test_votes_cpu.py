"""goi_raster_contrib_votes without a GPU: the numpy replay the GPU test compares the kernel with (tests/votes_reference.py)
against a plain float64 loop over the events of contrib_reference.pixel_loop, on test_contrib_cpu's random frames and its
saturating frame, under four label maps (uniform, a half-plane aligned to no multiple of 8, a 1-pixel checkerboard, 64 distinct
labels per quadrant) with and without ignored values; the selection rules of contrib.assign and contrib.lift_mask on hand-made
arrays; the entry's refusals by message; the header, the ctypes table and the ABI version; the refusal of CPU tensors.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import blend_reference as BR
from tests import contrib_reference as CR
from tests import test_contrib_cpu as TC
from tests import votes_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
NAME = "goi_raster_contrib_votes"
_FRAMES = {}


@pytest.fixture(autouse=True, scope="module")
def _the_replay_counts_in_the_products_unit():
    from goi_hyperplane_amd import contrib
    assert contrib.VOTE_ONE == VR.UNIT == 1 << 24


def _frames():
    """test_contrib_cpu's three random frames and its saturating frame -> name -> (fr, qd, alpha64, hit, events, tol)"""
    if _FRAMES:
        return _FRAMES
    rng = np.random.default_rng(5)
    made = []
    for W, H, n, radius in ((44, 27, 60, None), (12, 10, 25, None), (72, 40, 80, 20.0)):
        m, co = TC._random_records(rng, n, W, H)
        fr, qd, E, alpha, hit = BR.cpu_frame(W, H, m, co, np.zeros((n, 3)), rng.uniform(1, 9, n), np.zeros((n, 1)), np.zeros(3),
                                             radius=radius, dtype=np.float32)
        made.append((f"random-{W}x{H}", fr, qd, alpha, hit))
    fr, qd, alpha, hit, g_stop, pix = TC._saturating_frame(np.float32)
    made.append(("saturating", fr, qd, alpha, hit))
    for name, fr, qd, alpha, hit in made:
        alpha = alpha.astype(np.float64)
        events = CR.pixel_loop(fr, qd, alpha, hit)[3]
        tol = (2 * int(qd.length.max()) + 2) * 2.0 ** -24  # test_contrib_cpu's: the product chain's roundings
        tt = np.array([e[3] for e in events])
        assert (np.abs(tt - BR.T_MIN) > 4 * tol * BR.T_MIN).all(), "a stop decision of this fixture is marginal in fp32"
        _FRAMES[name] = (fr, qd, alpha, hit, events, tol)
    return _FRAMES


@pytest.mark.parametrize("ignored", [False, True])
@pytest.mark.parametrize("kind", VR.MAP_KINDS)
def test_replay_matches_the_loop(kind, ignored):
    for name, (fr, qd, alpha, hit, events, tol) in _frames().items():
        labels, K = VR.label_map(kind, fr.W, fr.H, ignored)
        if ignored:
            assert all((labels == v).any() for v in (-1, K, VR.INT_MAX, VR.INT_MIN)) or fr.W * fr.H < 200, name
        want, bound, cnt = VR.loop(events, labels, K, fr.P, tol)
        v64 = VR.votes(fr, qd, alpha, hit, labels, K, dtype=np.float64)
        assert v64.dtype == np.int64 and v64.shape == (fr.P, K)
        assert np.array_equal(v64, want), f"{name}: the float64 replay differs from the loop"
        v32 = VR.votes(fr, qd, alpha.astype(np.float32), hit, labels, K, dtype=np.float32)
        assert v32.dtype == np.int64
        assert (np.abs(v32 - want) <= bound).all(), f"{name}: fp32 replay off by {int(np.abs(v32 - want).max())} units"
        # total > 0 exactly for the Gaussians with a contributing event on a validly labelled pixel; every event is >= 1 unit
        assert np.array_equal(want > 0, cnt > 0) and np.array_equal(v32 > 0, cnt > 0) and (want >= cnt).all()
        assert (want.sum(1) > 0).any(), f"{name}: nothing voted"
        if kind == "half-plane":
            lab = VR.quad_labels(qd, labels, K)
            two = [(row[row >= 0] == 0).any() and (row[row >= 0] == 1).any() for row in lab]
            assert any(two), f"{name}: no quadrant holds two labels"


def test_ignored_labels_are_ignored_and_the_sums_are_the_contributions():
    fr, qd, alpha, hit, events, tol = _frames()["random-44x27"]
    labels, K = VR.label_map("checkerboard", fr.W, fr.H, True)
    v = VR.votes(fr, qd, alpha, hit, labels, K, dtype=np.float64)
    valid = (labels >= 0) & (labels < K)
    assert 0 < valid.sum() < valid.size
    total = sum(int(np.rint(e[2] * VR.UNIT)) for e in events if e[4] and valid[e[0]])
    assert int(v.sum()) == total
    # every ignored value behaves like every other: the same votes with all of them replaced by -1
    assert np.array_equal(v, VR.votes(fr, qd, alpha, hit, np.where(valid, labels, -1), K, dtype=np.float64))
    # K = 1 with everything valid: the row sums of any labelling
    all0 = VR.votes(fr, qd, alpha, hit, np.zeros(fr.W * fr.H, np.int32), 1, dtype=np.float64)
    full = VR.votes(fr, qd, alpha, hit, VR.label_map("64-distinct", fr.W, fr.H)[0], 64, dtype=np.float64)
    assert np.array_equal(full.sum(1), all0[:, 0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_stopper_does_not_vote(dtype):
    """The saturating frame's centre pixel alone is labelled: its five wide Gaussians vote their contributions, the sixth --
    which ends the pixel with the largest w it has anywhere -- votes nothing there, though it votes at the neighbours."""
    fr, qd, alpha, hit, events, tol = _frames()["saturating"]
    g_stop, pix = 5, 12 * fr.W + 20
    stops = [e for e in events if e[0] == pix and not e[4]]
    assert len(stops) == 1 and stops[0][1] == g_stop and stops[0][2] * VR.UNIT > 1000
    only = np.full(fr.W * fr.H, -1, np.int32)
    only[pix] = 0
    v = VR.votes(fr, qd, alpha.astype(dtype), hit, only, 1, dtype=dtype)
    assert v[g_stop, 0] == 0, "the stopper's weight must be absent"
    assert (v[:5, 0] > 0).all() and not v[6:].any()
    want, bound, _ = VR.loop(events, only, 1, fr.P, tol)
    assert (np.abs(v - want) <= (bound if dtype == np.float32 else 0)).all()
    everywhere = VR.votes(fr, qd, alpha.astype(dtype), hit, np.zeros(fr.W * fr.H, np.int32), 1, dtype=dtype)
    assert everywhere[g_stop, 0] > 0, "the sixth Gaussian contributes at the neighbouring pixels"


def test_assign_and_lift_rules_on_hand_made_votes():
    import torch
    from goi_hyperplane_amd import contrib
    one = contrib.VOTE_ONE
    assert one == 1 << 24 == VR.UNIT
    v = np.array([[5, 5, 1],        # a tie: the lowest class
                  [0, 7, 7],        # a tie among later classes
                  [0, 0, 0],        # no vote
                  [1, 2, 3],
                  [one, 0, one - 1],
                  [3, 0, 0],
                  [2 ** 40, 2 ** 40 + 1, 0],   # beyond float32's and (summed) close to float64's integers
                  [0, one // 2, one // 2 - 1]], np.int64)
    label, share = contrib._assign(torch.from_numpy(v), 0.0)
    assert label.dtype == torch.int64 and share.dtype == torch.float32
    assert label.tolist() == [0, 1, -1, 2, 0, 0, 1, 1]
    want_share = [5 / 11, 0.5, 0.0, 0.5, one / (2 * one - 1), 1.0, (2 ** 40 + 1) / (2 ** 41 + 1), (one // 2) / (one - 1)]
    assert share.tolist() == [float(np.float32(s)) for s in want_share]
    wl, ws = VR.assign(v)
    assert np.array_equal(label.numpy(), wl) and np.array_equal(share.numpy(), ws)
    # min_weight: strictly below min_weight * VOTE_ONE is -1 with share 0; exactly at it stays
    label, share = contrib._assign(torch.from_numpy(v), (one - 1) / one)
    assert label.tolist() == [-1, -1, -1, -1, 0, -1, 1, 1] and share[0] == 0 and share[7] > 0
    label, share = contrib._assign(torch.from_numpy(v), 1.0)
    assert label.tolist() == [-1, -1, -1, -1, 0, -1, 1, -1]
    wl, ws = VR.assign(v, 1.0)
    assert np.array_equal(label.numpy(), wl) and np.array_equal(share.numpy(), ws)

    m = np.array([[1, 1], [1, 2], [0, 0], [0, 1], [5, 0], [one, one + 1], [3 * one, one], [one // 2, one // 2]], np.int64)
    sel = contrib._lift(torch.from_numpy(m), 0.5, 0.0)
    assert sel.dtype == torch.bool
    assert sel.tolist() == [False, True, False, True, False, True, False, False]  # strictly more than threshold * total
    assert contrib._lift(torch.from_numpy(m), 0.25, 0.0).tolist() == [True, True, False, True, False, True, False, True]
    assert contrib._lift(torch.from_numpy(m), 0.5, 1.0).tolist() == [False, False, False, False, False, True, False, False]
    assert contrib._lift(torch.from_numpy(m), 0.0, 1.0).tolist() == [False, False, False, False, False, True, True, True]
    for thr, mw in ((0.5, 0.0), (0.25, 0.0), (0.5, 1.0), (0.0, 1.0)):
        assert np.array_equal(contrib._lift(torch.from_numpy(m), thr, mw).numpy(), VR.lift(m, thr, mw))
    with pytest.raises(ValueError, match="votes must be an int64 tensor"):
        contrib.assign(torch.zeros(3, 2))


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("args,message", [
    ((0, 16, 16, 1, F, F, F, F, 2, F, None), "goi_raster_contrib_votes: bad P/W/H/R"),
    ((10, 0, 16, 1, F, F, F, F, 2, F, None), "goi_raster_contrib_votes: bad P/W/H/R"),
    ((10, 16, -1, 1, F, F, F, F, 2, F, None), "goi_raster_contrib_votes: bad P/W/H/R"),
    ((10, 16, 16, -1, F, F, F, F, 2, F, None), "goi_raster_contrib_votes: bad P/W/H/R"),
    ((10, 16, 16, 1, None, F, F, F, 2, F, None), "goi_raster_contrib_votes: workspace pointer is NULL"),
    ((10, 16, 16, 1, F, None, F, F, 2, F, None), "goi_raster_contrib_votes: workspace pointer is NULL"),
    ((10, 16, 16, 1, F, F, None, F, 2, F, None), "goi_raster_contrib_votes: workspace pointer is NULL"),
    ((10, 16, 16, 0, F, None, None, F, 2, F, None), "goi_raster_contrib_votes: workspace pointer is NULL"),
    ((10, 16, 16, 1, F, F, F, None, 2, F, None), "goi_raster_contrib_votes: labels or votes is NULL"),
    ((10, 16, 16, 1, F, F, F, F, 2, None, None), "goi_raster_contrib_votes: labels or votes is NULL"),
    ((10, 16, 16, 0, F, None, F, None, 2, F, None), "goi_raster_contrib_votes: labels or votes is NULL"),
    ((10, 16, 16, 1, F, F, F, F, 0, F, None), "goi_raster_contrib_votes: K must be at least 1"),
    ((10, 16, 16, 0, F, None, F, F, -3, F, None), "goi_raster_contrib_votes: K must be at least 1"),
])
def test_the_entry_refuses_by_name(lib, args, message):
    assert getattr(lib, NAME)(*args) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_header_table_and_abi_version(lib):
    from goi_hyperplane_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    decl = re.search(r"int goi_raster_contrib_votes\(int P, int W, int H, int R, const void\* geom_buffer, const void\* binning_buffer,"
                     r"\s*const void\* image_buffer, const int\* labels /\*\[H\*W\]\*/, int K,"
                     r"\s*int64_t\* votes /\*\[P\*K\], added to\*/, void\* stream\);", hdr)
    assert decl, "the entry is not declared with the documented signature"
    version = re.search(r"#define GOI_RASTER_ABI_VERSION (\d+)", hdr)
    nine = hdr.index("\n/* 9:")
    eight = hdr.index("\n * 8:")
    assert nine < hdr.index(NAME) < eight < version.start() < decl.start(), "must be named among ABI 9's later additions, above the version"
    assert "later additions" in hdr[nine:hdr.index(NAME)]
    assert int(version.group(1)) == 9 == _lib.ABI_VERSION == lib.goi_raster_abi_version()
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int and argtypes == [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 2
    assert hasattr(lib, NAME)
    from goi_hyperplane_amd import contrib
    for fn in ("votes_buffers", "frame_votes", "votes", "assign", "lift_mask", "VOTE_ONE"):
        assert hasattr(contrib, fn), fn


def test_cpu_tensors_are_refused():
    import torch
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import make_camera, make_scene
    pc = GaussianSet.from_scene(make_scene(10, S=16, sh_degree=1, seed=0), "cpu")
    cam = TorchCamera(make_camera(16, 16), "cpu")
    bg = torch.zeros(3)
    lab = torch.zeros(16, 16, dtype=torch.int32)
    z = torch.zeros(8)
    for call in (lambda: contrib.frame_votes(cam, pc, bg, lab, 2), lambda: contrib.votes([cam], pc, bg, [lab], 2),
                 lambda: contrib.lift_mask([cam], pc, bg, lab[None] != 0), lambda: contrib.assign(torch.zeros(10, 2, dtype=torch.int64)),
                 lambda: contrib.votes_buffers(10, 16, 16, 0, z, z, z, lab, 2)):
        with pytest.raises(RuntimeError, match="goi_hyperplane_amd.contrib: tensors must live on a ROCm GPU; there is no CPU fallback"):
            call()
