"""One small scene and camera for every semantic width S = 1..32 (tests/test_channel_counts_cpu.py proves its properties on the
CPU, tests/test_gpu_channel_counts.py and tests/test_gpu_blend_rows.py put it through the frame kernels at every width), and
the dispatch classes of a width restated from the headers.  numpy only.

case(S): the same Gaussians and the same camera at every width; the semantics are the first S columns of ONE seeded [P, 32]
table, so that channel k of the width-S frame can be compared bit for bit with channel k of the width-32 frame.  The scene is
three make_scene() populations seen by one make_camera() at 83 x 69 (6 x 5 tiles, 3 and 5 pixels into the last column and row
of tiles: ragged quadrants and quadrants wholly outside the image):
  * 240 small Gaussians over the usual box: short lists, tiles with fewer than 8 entries, untouched pixels along the borders;
  * a BLOB of 110 large Gaussians around one point: lists longer than 64 entries (two staging rounds of the blend), pixels that
    saturate and stop early, Gaussians listed in dozens of tiles;
  * a HAZE of 110 large Gaussians of opacity 0.006 .. 0.054 around another: pixels with more than 64 contributors that never
    saturate (a last contributor in the second round).

Measured on one CPU core: one evaluation of the float64 row reference (tests/blend_reference.py::backward_rows; 8 904 candidate
pairs, 2 243 member rows, up to 99 contributors deep) takes 0.07 - 0.10 s, the oracle's forward + backward 0.02 - 0.05 s, at any
width (docs/MEASUREMENT_LOG.md, "Every semantic width 1..32 through the frame kernels").
"""
from __future__ import annotations

import functools

import numpy as np

from goi_hyperplane_amd.scene import GaussianScene, make_camera, make_scene

WIDTHS = tuple(range(1, 33))
W, H = 83, 69
BG = np.array([0.1, 0.3, 0.6], np.float32)
N_SMALL, N_BLOB, N_HAZE = 240, 110, 110
# The forms of the backward blend besides the default run on two widths per S4 class: the 16-byte row path and the scalar one.
PAIRED_WIDTHS = tuple(w for s4 in range(1, 9) for w in (4 * s4 - 1, 4 * s4))


# ---- the dispatch rules, restated (csrc/blend_common.h: GOI_DISPATCH_S4; csrc/common.h: bwd_row_floats, bwd_sem_row_floats;
# the kernels' `(S & 3) == 0` and `(S & 1) == 0` tests).  tests/test_channel_counts_cpu.py checks them against the sources.
def s4_of(S: int) -> int:
    return (S + 3) // 4


def nsem_of(S: int) -> int:
    return 4 * s4_of(S)


def nb_of(S: int) -> int:
    """accumulator blocks of 16 columns of the padded channels"""
    return (nsem_of(S) + 15) // 16


def bwd_row_floats(S: int) -> int:
    return ((nsem_of(S) + 10 + 15) // 16) * 16


def bwd_sem_row_floats(S: int) -> int:
    return ((nsem_of(S) + 15) // 16) * 16


def dispatch_class(S: int) -> dict:
    return dict(S4=s4_of(S), mod4=S % 4, even=S % 2 == 0, vector_rows=S % 4 == 0, wide_launch_bounds=s4_of(S) > 4, NB=nb_of(S),
                row_floats=bwd_row_floats(S), sem_row_floats=bwd_sem_row_floats(S),
                rows_in_preprocess=bwd_row_floats(S) == 32)


# ---- the scene -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _geometry():
    small = make_scene(N_SMALL, S=1, sh_degree=1, seed=41, log_scale_mean=-3.0)
    blob = make_scene(N_BLOB, S=1, sh_degree=1, seed=42, log_scale_mean=-2.0, extent=(0.30, 0.25, 0.3))
    haze = make_scene(N_HAZE, S=1, sh_degree=1, seed=43, log_scale_mean=-1.8, extent=(0.25, 0.25, 0.3))
    blob.means3D += np.array([0.9, -0.5, 0.0], np.float32)
    haze.means3D += np.array([-1.0, 0.6, 0.0], np.float32)
    haze.opacities *= np.float32(0.06)
    parts = (small, blob, haze)
    cat = lambda name: np.ascontiguousarray(np.concatenate([getattr(p, name) for p in parts]))  # noqa: E731
    table = np.random.default_rng(44).normal(size=(N_SMALL + N_BLOB + N_HAZE, 32)).astype(np.float32)
    return {k: cat(k) for k in ("means3D", "scales", "rotations", "opacities", "shs")}, table


def semantics_table() -> np.ndarray:
    """[P, 32]: case(S).semantics is its first S columns"""
    return _geometry()[1]


def case(S: int):
    """(scene, camera) of width S in 1..32"""
    if not 1 <= S <= 32:
        raise ValueError("S must be in 1..32")
    g, table = _geometry()
    sc = GaussianScene(g["means3D"].copy(), g["scales"].copy(), g["rotations"].copy(), g["opacities"].copy(), g["shs"].copy(),
                       np.ascontiguousarray(table[:, :S]), 1, meta=dict(S=S))
    return sc, make_camera(W, H, yaw=0.2, pitch=-0.1)


def upstream(S: int):
    """(dL_dcolor [3,H,W], dL_dsem [S,H,W], dL_ddepth [1,H,W], dL_dalpha [1,H,W]) of width S: the semantic part is the first S
    maps of one seeded [32, H, W] table, like the semantics."""
    rng = np.random.default_rng(45)
    n = lambda *shape: rng.normal(size=shape).astype(np.float32)  # noqa: E731
    c, s, d, a = n(3, H, W), n(32, H, W), n(1, H, W), n(1, H, W)
    return c, np.ascontiguousarray(s[:S]), d, a


def upstream_dict(S: int) -> dict:
    c, s, d, a = upstream(S)
    return dict(color=c, sem=s, depth=d[0], alpha=a[0])


# ---- the oracle's run of a width: computed once, shared by every test that asks (read-only) -------------------------------------
_ORACLE = {}


def oracle_reference(S: int) -> dict:
    """dict(forward = oracle ForwardResult, state = its forward state, grads = its backward under upstream(S))"""
    if S not in _ORACLE:
        from oracle import oracle
        oracle.build()
        sc, cam = case(S)
        o = oracle.from_scene(sc, cam, bg=BG)
        f = o.forward()
        st = o.state()
        g = o.backward(*upstream(S))
        for a in list(st.values()) + list(g.values()) + [f.color, f.semantic, f.depth, f.alpha, f.radii, f.fragile]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ORACLE[S] = dict(forward=f, state=st, grads=g)
    return _ORACLE[S]
