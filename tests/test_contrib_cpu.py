"""goi_raster_contrib_frame without a GPU: the numpy replay the GPU test compares the kernel with (tests/contrib_reference.py)
against a plain per-pixel float64 loop of the same rule, on frames made by blend_reference.cpu_frame -- random Gaussians, a
pixel that saturates (a stopper whose w is larger than any contribution of its Gaussian elsewhere) and two equal weights in
one pixel; the entry's refusals by message; the header, the ctypes table and the ABI version.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import blend_reference as BR
from tests import contrib_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
NAME = "goi_raster_contrib_frame"


def _random_records(rng, n, W, H, sigma=(1.0, 6.0), opacity=(0.05, 0.95)):
    s = rng.uniform(*sigma, n)
    m = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    co = np.stack([1 / s ** 2, np.zeros(n), 1 / s ** 2, rng.uniform(*opacity, n)], 1)
    return m, co


def _saturating_frame(dtype):
    """40 random Gaussians behind/around a stack over pixel (20, 12) of a 44 x 27 image (ragged in both directions): five wide
    Gaussians of opacity 0.8 and, behind them, a NARROW sixth of opacity 0.8 that ends the pixel -- T there is 0.2^5 = 3.2e-4, so
    its w = 2.56e-4 while T (1 - alpha) = 6.4e-5 < 1e-4; at the neighbouring pixels it is faint and contributes less."""
    W, H = 44, 27
    rng = np.random.default_rng(11)
    m, co = _random_records(rng, 40, W, H)
    depths = rng.uniform(6.0, 9.0, 40)
    wide = np.array([[20.0, 12.0]] * 5)
    m = np.concatenate([wide, [[20.0, 12.0]], m])
    co = np.concatenate([np.tile([1 / 36.0, 0.0, 1 / 36.0, 0.8], (5, 1)), [[1 / 0.3, 0.0, 1 / 0.3, 0.8]], co])
    depths = np.concatenate([1.0 + 0.1 * np.arange(5), [2.0], depths])
    P = len(depths)
    fr, qd, E, alpha, hit = BR.cpu_frame(W, H, m, co, np.zeros((P, 3)), depths, np.zeros((P, 1)), np.zeros(3), dtype=dtype)
    return fr, qd, alpha, hit, 5, 12 * W + 20


def _check_against_loop(fr, qd, alpha, hit):
    """replay in float64 == the plain loop, exactly; replay in float32 within the product chain's roundings of it (the frames
    are made so that no stop decision sits within that distance of 1e-4)."""
    peak, tid, tw, events = CR.pixel_loop(fr, qd, alpha, hit)
    p64, i64, w64 = CR.replay(fr, qd, alpha, hit, dtype=np.float64)
    assert np.array_equal(p64, peak) and np.array_equal(i64, tid) and np.array_equal(w64, tw)
    K = int(qd.length.max())
    tol = (2 * K + 2) * 2.0 ** -24
    tt = np.array([e[3] for e in events])
    assert (np.abs(tt - BR.T_MIN) > 4 * tol * BR.T_MIN).all(), "a stop decision of this fixture is marginal in fp32"
    p32, i32, w32 = CR.replay(fr, qd, alpha.astype(np.float32), hit, dtype=np.float32)
    assert p32.dtype == np.float32 and w32.dtype == np.float32 and i32.dtype == np.int32
    assert (np.abs(p32 - peak) <= tol * peak).all() and (np.abs(w32 - tw) <= tol * tw).all()
    # the dominant contributor may differ only where the two best weights of a pixel are within the roundings of each other
    differ = np.flatnonzero(i32 != tid)
    for pix in differ:
        ws = sorted((e[2] for e in events if e[0] == pix and e[4]), reverse=True)
        assert len(ws) >= 2 and ws[0] - ws[1] <= 2 * tol * ws[0], (int(pix), ws[:2])
    return peak, tid, tw, events


def test_replay_matches_the_pixel_loop_on_random_frames():
    rng = np.random.default_rng(5)
    for W, H, n, radius in ((44, 27, 60, None), (12, 10, 25, None), (72, 40, 80, 20.0)):
        m, co = _random_records(rng, n, W, H)
        fr, qd, E, alpha, hit = BR.cpu_frame(W, H, m, co, np.zeros((n, 3)), rng.uniform(1, 9, n), np.zeros((n, 1)), np.zeros(3),
                                             radius=radius, dtype=np.float32)
        peak, tid, tw, events = _check_against_loop(fr, qd, alpha.astype(np.float64), hit)
        assert (tid >= 0).any() and (peak > 0).any()
        # outside the image nothing is live; a Gaussian with no event has peak 0
        seen = np.zeros(n, bool)
        seen[[e[1] for e in events]] = True
        assert not peak[~seen].any() and (peak[seen] > 0).all()


def test_the_stopper_counts_for_peak_and_not_for_top():
    fr, qd, alpha, hit, g_stop, pix = _saturating_frame(np.float32)
    peak, tid, tw, events = _check_against_loop(fr, qd, alpha.astype(np.float64), hit)
    stops = [e for e in events if e[0] == pix and not e[4]]
    assert len(stops) == 1 and stops[0][1] == g_stop, "the sixth Gaussian must end the centre pixel"
    w_stop = stops[0][2]
    contributions = [e[2] for e in events if e[1] == g_stop and e[4]]
    assert contributions and w_stop > max(contributions), "the stopper's w must exceed every contribution of its Gaussian"
    assert peak[g_stop] == w_stop
    # the pixel's dominant contributor is the front-most wide Gaussian (w = its alpha), not the stopper
    assert tid[pix] == 0 and tw[pix] == float(alpha_of(fr, qd, alpha, 0, pix))
    p32, i32, w32 = CR.replay(fr, qd, alpha, hit)
    assert i32[pix] == 0 and w32[pix] == alpha_of(fr, qd, alpha, 0, pix)
    assert p32[g_stop] == np.float32(alpha_of(fr, qd, alpha, g_stop, pix) * chain_T(fr, qd, alpha, hit, pix, 5))


def alpha_of(fr, qd, alpha, g, pix):
    q, lane = np.argwhere((qd.pix == pix) & qd.inside)[0]
    pos = int(np.flatnonzero(qd.pair_id[qd.off[q]:qd.off[q + 1]] == g)[0])
    return alpha[qd.off[q] + pos, lane]


def chain_T(fr, qd, alpha, hit, pix, n):
    """fp32 transmittance of `pix` after its first n hits"""
    q, lane = np.argwhere((qd.pix == pix) & qd.inside)[0]
    T, k = np.float32(1), 0
    for pos in range(int(qd.length[q])):
        i = qd.off[q] + pos
        if hit[i, lane] and k < n:
            T = np.float32(T * np.float32(np.float32(1) - np.float32(alpha[i, lane])))
            k += 1
    return T


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_front_most_of_two_equal_weights_wins(dtype):
    """Two Gaussians over every pixel of one tile with per-candidate alphas set by hand: a1, and an a2 found by search such that
    a2 * (1 - a1) rounds to a1 exactly in `dtype` -- the pixel's two weights are equal, the first in list order is reported.
    A third, larger weight behind them on some pixels still takes over (strict >)."""
    m = np.array([[8.0, 8.0]] * 3)
    co = np.tile([1e-4, 0.0, 1e-4, 0.5], (3, 1))
    fr, qd, E, alpha, hit = BR.cpu_frame(16, 16, m, co, np.zeros((3, 3)), np.array([1.0, 2.0, 3.0]), np.zeros((3, 1)), np.zeros(3), dtype=dtype)
    assert qd.npairs == 12 and hit.all()
    rng = np.random.default_rng(2)
    found = None
    for a1 in rng.uniform(0.15, 0.3, 4000).astype(dtype):
        T1 = dtype(dtype(1) - a1)
        a2 = dtype(a1 / T1)
        for _ in range(8):
            if dtype(a2 * T1) == a1:
                found = (a1, a2)
                break
            a2 = np.nextafter(a2, dtype(0) if dtype(a2 * T1) > a1 else dtype(1)).astype(dtype)
        if found:
            break
    assert found, "no exact tie found"
    a1, a2 = found
    alpha = np.zeros((12, 64), dtype)
    pos = qd.pair_pos
    alpha[pos == 0], alpha[pos == 1] = a1, a2
    third = np.zeros(64, dtype)
    third[:32] = 0.9  # w3 = 0.9 (1 - a1)(1 - a2) > a1 on the first 32 lanes of every quadrant
    alpha[pos == 2] = third
    hit = alpha > 0
    peak, tid, tw = CR.replay(fr, qd, alpha, hit, dtype=dtype)
    q_lane = np.zeros((qd.Q, 64), bool)
    q_lane[:, :32] = True
    big = np.zeros(256, bool)
    big[qd.pix[q_lane]] = True
    assert (tid[~big] == 0).all() and (tw[~big] == a1).all(), "the front-most of two equal weights must win"
    assert (tid[big] == 2).all() and (tw[big] > a1).all()
    assert peak[0] == a1 and peak[1] == a1 and peak[2] == tw[big].max()
    if dtype == np.float64:
        lp, li, lw, _ = CR.pixel_loop(fr, qd, alpha, hit)
        assert np.array_equal(lp, peak) and np.array_equal(li, tid) and np.array_equal(lw, tw)


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("args,message", [
    ((0, 16, 16, 1, F, F, F, F, F, F, None), "goi_raster_contrib_frame: bad P/W/H/R"),
    ((10, 0, 16, 1, F, F, F, F, F, F, None), "goi_raster_contrib_frame: bad P/W/H/R"),
    ((10, 16, -1, 1, F, F, F, F, F, F, None), "goi_raster_contrib_frame: bad P/W/H/R"),
    ((10, 16, 16, -1, F, F, F, F, F, F, None), "goi_raster_contrib_frame: bad P/W/H/R"),
    ((10, 16, 16, 1, None, F, F, F, F, F, None), "goi_raster_contrib_frame: workspace pointer is NULL"),
    ((10, 16, 16, 1, F, None, F, F, F, F, None), "goi_raster_contrib_frame: workspace pointer is NULL"),
    ((10, 16, 16, 1, F, F, None, F, F, F, None), "goi_raster_contrib_frame: workspace pointer is NULL"),
    ((10, 16, 16, 0, F, None, None, F, F, F, None), "goi_raster_contrib_frame: workspace pointer is NULL"),
    ((10, 16, 16, 1, F, F, F, None, None, None, None), "goi_raster_contrib_frame: peak, top_id and top_w are all NULL"),
])
def test_the_entry_refuses_by_name(lib, args, message):
    assert getattr(lib, NAME)(*args) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_header_table_and_abi_version(lib):
    from goi_hyperplane_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    decl = re.search(r"int goi_raster_contrib_frame\(int P, int W, int H, int R, const void\* geom_buffer, const void\* binning_buffer,"
                     r"\s*const void\* image_buffer, float\* peak, int\* top_id, float\* top_w, void\* stream\);", hdr)
    assert decl, "the entry is not declared with the documented signature"
    version = re.search(r"#define GOI_RASTER_ABI_VERSION (\d+)", hdr)
    assert hdr.index(NAME) < version.start() < decl.start(), "must be named among ABI 8's later additions, above the version"
    assert int(version.group(1)) == 9 == _lib.ABI_VERSION == lib.goi_raster_abi_version()
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int and argtypes == [C.c_int] * 4 + [C.c_void_p] * 7
    assert hasattr(lib, NAME)
    from goi_hyperplane_amd import contrib
    for fn in ("frame", "peak_weights", "pick", "prune_unseen", "ContribFrame"):
        assert hasattr(contrib, fn), fn


def test_cpu_tensors_are_refused():
    import torch
    from goi_hyperplane_amd import contrib
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import make_camera, make_scene
    pc = GaussianSet.from_scene(make_scene(10, S=16, sh_degree=1, seed=0), "cpu")
    cam = TorchCamera(make_camera(16, 16), "cpu")
    bg = torch.zeros(3)
    for call in (lambda: contrib.frame(cam, pc, bg), lambda: contrib.peak_weights([cam], pc, bg),
                 lambda: contrib.pick(cam, pc, bg, (3, 4)), lambda: contrib.prune_unseen(pc, [cam], bg)):
        with pytest.raises(RuntimeError, match="goi_hyperplane_amd.contrib: tensors must live on a ROCm GPU; there is no CPU fallback"):
            call()
