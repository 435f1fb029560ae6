"""The scenes and upstream gradients on which the blend kernels are tested directly (tests/test_gpu_blend_rows.py) and on which
the float32 yardstick of their tolerance is measured (tools/blend_yardstick.py, docs/MEASUREMENT_LOG.md).  numpy only.

Row cases: S in {1, 3, 4, 10, 16, 17, 20, 32} (every S4 instantiation class, the register path of S % 4 != 0, both occupancy
classes), a ragged image, W, H = 8 mod 16 (quadrants wholly outside the image), an image smaller than a tile, the parity suite's
huge-Gaussian scene (long lists) and its 300-Gaussian scene (rectangles beyond the 64-tile masks), a camera inside the cloud, and
constructed STACKS of K equal-footprint Gaussians over one quadrant at opacity 0.02 (K around the flush group of 8, the batch of 32,
the forward round of 64 and the carry across them) and at 0.99 (saturation, tiny T_final).
"""
from __future__ import annotations

import math
import zlib

import numpy as np

from goi_hyperplane_amd.scene import GaussianScene, make_camera, make_scene

BG0 = np.zeros(3, np.float32)
BG1 = np.array([0.3, 0.7, 0.1], np.float32)
STACK_K = (1, 7, 8, 9, 31, 32, 33, 40, 63, 64, 65, 129)


def seed_of(tag: str) -> int:
    return zlib.crc32(tag.encode())


def stack_scene(K: int, opacity: float, S: int = 16, W: int = 48, H: int = 32, centre=(20.0, 12.0), sigma_px: float = 2.5):
    """K isotropic Gaussians of one footprint (sigma_px pixels) centred on one pixel position, 0.01 apart in depth."""
    cam = make_camera(W, H)
    rng = np.random.default_rng(seed_of(f"stack/{K}/{opacity}/{S}"))
    zc = 5.0 + 0.01 * np.arange(K)
    ndc_x, ndc_y = (2 * centre[0] + 1) / W - 1, (2 * centre[1] + 1) / H - 1
    xyz = np.stack([ndc_x * zc * cam.tanfovx, ndc_y * zc * cam.tanfovy, zc - 5.0], 1).astype(np.float32)
    focal = W / (2 * cam.tanfovx)
    scales = np.repeat((sigma_px * zc / focal)[:, None], 3, 1).astype(np.float32)
    rot = np.zeros((K, 4), np.float32)
    rot[:, 0] = 1
    sc = GaussianScene(xyz, scales, rot, np.full((K, 1), opacity, np.float32),
                       rng.normal(0, 0.5, (K, 1, 3)).astype(np.float32), rng.normal(0, 1, (K, S)).astype(np.float32), 0)
    return sc, cam


def _rand(P, S, W, H, mu, deg=1, seed=3, **cam):
    return lambda: (make_scene(P, S=S, sh_degree=deg, seed=seed, log_scale_mean=mu), make_camera(W, H, **cam))


def _inside():
    sc = make_scene(3000, S=16, sh_degree=1, seed=3, log_scale_mean=-3.0, extent=(2.0, 1.5, 1.0))
    return sc, make_camera(160, 120, yaw=0.3, pitch=-0.1, distance=1.0, target=(0.0, 0.0, 0.5))


# name -> () -> (scene, camera)
ROW_CASES = {f"S{S}": _rand(600, S, 96, 80, -2.5, yaw=0.2, pitch=-0.1) for S in (1, 3, 4, 10, 16, 17, 20, 32)}
ROW_CASES.update({
    "ragged-123x77": _rand(1500, 16, 123, 77, -2.6, deg=2, yaw=0.2, pitch=-0.1),
    "8mod16-72x40": _rand(500, 10, 72, 40, -2.5),
    "sub-tile-12x10": _rand(200, 16, 12, 10, -2.0),
    "huge-64x48": _rand(800, 16, 64, 48, -1.2, yaw=0.2, pitch=-0.1),
    "masks-400x300": _rand(300, 16, 400, 300, -0.6, deg=2, yaw=0.2, pitch=-0.1),
    "inside-160x120": _inside,
})
for _K in STACK_K:
    ROW_CASES[f"stack-{_K}"] = (lambda K=_K: stack_scene(K, 0.02))
    ROW_CASES[f"opaque-{_K}"] = (lambda K=_K: stack_scene(K, 0.99))

UPSTREAM_BASE = "S10"  # the scene the upstream-gradient cases run on
UPSTREAM_KINDS = ("random", "one-hot", "zero-channel", "2^+-40", "2^20-range", "color-only", "sem-only", "depth-only", "alpha-only",
                  "bg")


def upstream(kind: str, S: int, H: int, W: int, tag: str) -> tuple[dict, np.ndarray]:
    """(dict(color [3,H,W], sem [S,H,W], depth [H,W], alpha [H,W]; None: absent), bg) of an upstream-gradient case."""
    rng = np.random.default_rng(seed_of(f"up/{kind}/{tag}"))
    n = lambda *shape: rng.normal(size=shape).astype(np.float32)  # noqa: E731
    up = dict(color=n(3, H, W), sem=n(S, H, W), depth=n(H, W), alpha=n(H, W))
    bg = BG0
    if kind == "random":
        pass
    elif kind == "one-hot":
        keep = up["sem"][S // 2].copy()
        up = dict(color=np.zeros((3, H, W), np.float32), sem=np.zeros((S, H, W), np.float32), depth=np.zeros((H, W), np.float32),
                  alpha=np.zeros((H, W), np.float32))
        up["sem"][S // 2] = keep
    elif kind == "zero-channel":
        up["sem"][0] = 0
        up["color"][1] = 0
    elif kind == "2^+-40":
        up["sem"][0] *= np.float32(2.0 ** 40)
        up["sem"][S - 1] *= np.float32(2.0 ** -40)
        up["color"][2] *= np.float32(2.0 ** -40)
    elif kind == "2^20-range":  # inside ONE channel of ONE quadrant: the split operand's scale follows the largest value
        up["sem"][S // 2, 8:16, 16:24] *= np.exp2(rng.uniform(0, 20, (8, 8))).astype(np.float32)
        up["color"][0, 8:16, 16:24] *= np.exp2(rng.uniform(0, 20, (8, 8))).astype(np.float32)
    elif kind.endswith("-only"):
        only = kind[:-5]
        up = {k: (v if k == only else None) for k, v in up.items()}
    elif kind == "bg":
        bg = BG1
    else:
        raise ValueError(kind)
    return up, bg


def all_runs():
    """(case name, upstream kind) of every backward-row run: every row case under random gradients, the base scene under the others."""
    return [(name, "random") for name in ROW_CASES] + [(UPSTREAM_BASE, k) for k in UPSTREAM_KINDS if k != "random"]


# ---- pair-evaluation cases: records written directly (no scene) -----------------------------------------------------------------
def pair_cases(W: int = 70, H: int = 40):
    """(means2D [P,2], conic_opacity [P,4]) fp32 records for the pair-evaluation test: Gaussians on both sides of the S = 16 switch
    of poly_coefs, needles hundreds of pixels long, opacity 0 and just below / above 1/255, centres inside a quadrant (power ~ 0
    against kPowerTol), the sharpest admissible conic a = c = 1/0.3.  Every one is requested against every quadrant, the partly
    and wholly outside ones of a 70 x 40 image included."""
    rng = np.random.default_rng(seed_of("pairs"))
    m, co = [], []

    def add(x, y, a, b, c, o):
        m.append((x, y))
        co.append((a, b, c, o))

    for _ in range(40):  # round Gaussians of every size, anywhere (also outside the image)
        s = math.exp(rng.uniform(math.log(0.6), math.log(60)))
        add(rng.uniform(-20, W + 20), rng.uniform(-20, H + 20), 1 / s ** 2, 0.0, 1 / s ** 2, rng.uniform(0.01, 1.0))
    for _ in range(40):  # anisotropic, rotated
        s1, s2 = math.exp(rng.uniform(math.log(0.6), math.log(40))), math.exp(rng.uniform(math.log(0.6), math.log(40)))
        th = rng.uniform(0, math.pi)
        c_, s_ = math.cos(th), math.sin(th)
        a = c_ * c_ / s1 ** 2 + s_ * s_ / s2 ** 2
        c = s_ * s_ / s1 ** 2 + c_ * c_ / s2 ** 2
        b = c_ * s_ * (1 / s1 ** 2 - 1 / s2 ** 2)
        add(rng.uniform(0, W), rng.uniform(0, H), a, b, c, rng.uniform(0.05, 1.0))
    for L in (100.0, 300.0, 800.0):  # needles: thin across (0.6 px), L pixels along, at several angles, passing through the image
        for th in (0.0, 0.3, math.pi / 4, 1.2, math.pi / 2):
            c_, s_ = math.cos(th), math.sin(th)
            s1, s2 = L, 0.6
            a = c_ * c_ / s1 ** 2 + s_ * s_ / s2 ** 2
            c = s_ * s_ / s1 ** 2 + c_ * c_ / s2 ** 2
            b = c_ * s_ * (1 / s1 ** 2 - 1 / s2 ** 2)
            t = rng.uniform(-0.5, 0.5) * L
            add(W / 2 + t * c_, H / 2 + t * s_, a, b, c, 0.8)
    for d in np.linspace(3.0, 5.0, 21):  # S = a D^2 sweeps through 16 at quadrant (0, 0), whose centre is (3.5, 3.5)
        add(3.5 + d, 3.5, 1.0, 0.0, 1.0, 0.9)
    add(3.5 + 4.0, 3.5, 1.0, 0.0, 1.0, 0.9)            # S = 16 exactly
    add(3.5 + 2.0, 3.5 + 2.0, 2.0, 0.0, 2.0, 0.9)      # S = 16 exactly
    for o in (0.0, 1 / 255 - 1e-6, float(np.float32(1) / np.float32(255)), 1 / 255 + 1e-6, 0.00392, 0.00393, 1.0):
        add(19.0, 11.0, 0.2, 0.0, 0.2, o)              # centre ON a pixel: power = 0 there
        add(19.0 + 1e-3, 11.0 - 1e-3, 0.2, 0.05, 0.2, o)
    for x, y in ((19.0, 11.0), (19.5, 11.5), (16.0, 8.0), (23.0, 15.0), (19.00001, 11.0), (3.5, 3.5)):
        add(x, y, 1 / 0.3, 0.0, 1 / 0.3, 0.99)         # the sharpest admissible conic, centre in / on pixels of a quadrant
        add(x, y, 0.01, 0.0, 0.01, 0.5)
    return np.array(m, np.float32), np.array(co, np.float32), W, H
