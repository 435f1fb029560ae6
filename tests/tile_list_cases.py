"""The committed case list of the tile-list tests (tests/test_tile_lists_cpu.py, tests/test_gpu_tile_lists.py): hand-built
scenes that realise the edges of the culled tile lists, a seeded sweep and the three large tile grids.  TEST INFRASTRUCTURE ONLY.

Hand-built scenes use the canonical camera (yaw = pitch = 0: W2C = [I | (0, 0, 5)]), so a Gaussian is placed at a pixel and a view
depth by inverting the projection (`place`), equal world z means bit-equal view depth, and an axis-aligned Gaussian with a
negligible z scale has cov2D = diag((f s_x / z)^2, (f s_y / z)^2) + 0.3.  What a case actually hits is not taken on trust: the
CPU test counts every coverage class from the oracle's state and the float64 reference."""
from __future__ import annotations

import math

import numpy as np

from goi_hyperplane_amd.scene import make_camera, make_clustered_scene, make_scene

Z = 5.0  # view depth of the hand-placed Gaussians unless said otherwise
INV255 = np.float32(1.0) / np.float32(255.0)


def focal(cam):
    return cam.image_width / (2.0 * cam.tanfovx)


def place(cam, px, py, z=Z):
    """World position that projects to pixel (px, py) at view depth z under the canonical camera."""
    px, py, z = np.broadcast_arrays(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(z, np.float64))
    x = z * cam.tanfovx * ((2.0 * px + 1.0) / cam.image_width - 1.0)
    y = z * cam.tanfovy * ((2.0 * py + 1.0) / cam.image_height - 1.0)
    return np.stack([x, y, z - 5.0], axis=-1).astype(np.float32)


def _blank(P, seed, S=4):
    sc = make_scene(P, S=S, sh_degree=1, seed=seed)
    sc.rotations[:] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    sc.scales[:] = 1e-4
    sc.opacities[:] = 0.5
    return sc


def _set_sigma_px(sc, cam, idx, sx, sy, z=Z):
    """Scales such that the Gaussian's pixel-space sigmas (before the 0.3 dilation) are sx, sy."""
    sc.scales[idx, 0] = np.asarray(sx) * np.asarray(z) / focal(cam)
    sc.scales[idx, 1] = np.asarray(sy) * np.asarray(z) / focal(cam)


def _rot_z(theta):
    theta = np.asarray(theta, np.float64)
    q = np.zeros(theta.shape + (4,), np.float32)
    q[..., 0] = np.cos(0.5 * theta)
    q[..., 3] = np.sin(0.5 * theta)
    return q


def tau_of(o):
    return 1.01 * math.log(255.0 * o) + 0.01


# ------------------------------------------------------------------------------------------------------------ hand-built
def opacity_edges():
    """Opacities at, just above and just below 1/255 (tau near 0.01), up to 1.01 / 255, and exactly 1.0."""
    W, H = 400, 300
    cam = make_camera(W, H)
    P = 1600
    sc = _blank(P, 41)
    rng = np.random.default_rng(41)
    sc.means3D[:] = place(cam, rng.uniform(-10, W + 10, P), rng.uniform(-10, H + 10, P), rng.uniform(3.0, 8.0, P))
    s = np.exp(rng.normal(1.6, 0.7, (P, 2)))
    _set_sigma_px(sc, cam, np.arange(P), s[:, 0], s[:, 1], sc.means3D[:, 2] + 5.0)
    sc.rotations[:] = _rot_z(rng.uniform(0, np.pi, P))
    lo = np.float32(INV255)
    vals = [lo, np.nextafter(lo, np.float32(1)), np.nextafter(lo, np.float32(0)), np.float32(lo * np.float32(1.004)),
            np.float32(lo * np.float32(1.0095)), np.float32(1.0), np.float32(0.9) * lo, np.float32(0.999) * lo,
            np.float32(0.5), np.float32(0.004), np.float32(0.0041), np.float32(0.05)]
    sc.opacities[:, 0] = np.array(vals, np.float32)[np.arange(P) % len(vals)]
    return sc, cam


def needles(seed=43, W=400, H=300, n_far=40, n_mid=700):
    """Diagonal needles: the longest (sigma of several hundred to tens of thousands of pixels) have a conic that cancels
    (determinant within 1e-5 relative of zero, or not positive at all in fp32: no finite box), the shorter ones are where the
    ellipse test removes most of the box."""
    cam = make_camera(W, H)
    P = n_far + n_mid
    sc = _blank(P, seed)
    rng = np.random.default_rng(seed)
    z = rng.uniform(3.0, 8.0, P)
    sc.means3D[:] = place(cam, rng.uniform(0, W, P), rng.uniform(0, H, P), z)
    long_px = np.concatenate([np.exp(rng.uniform(np.log(400.0), np.log(40000.0), n_far)),
                              np.exp(rng.uniform(np.log(6.0), np.log(90.0), n_mid))])
    thin_px = np.exp(rng.uniform(np.log(0.05), np.log(1.5), P))
    _set_sigma_px(sc, cam, np.arange(P), long_px, thin_px, z)
    ang = np.where(rng.uniform(size=P) < 0.6, np.pi / 4 * rng.choice([1, 3], P) + rng.normal(0, 0.02, P), rng.uniform(0, np.pi, P))
    sc.rotations[:] = _rot_z(ang)
    sc.opacities[:, 0] = np.exp(rng.uniform(np.log(0.9 / 255), 0.0, P)).astype(np.float32)
    order = rng.permutation(P)  # the degenerate ones are spread over the ids
    for name in ("means3D", "scales", "rotations", "opacities"):
        setattr(sc, name, np.ascontiguousarray(getattr(sc, name)[order]))
    return sc, cam


def tile_borders():
    """Centres on tile borders (pixel 16 k, 16 k - 0.5, 16 k - 1, 16 k + 15 in x and / or y) and outside the image on each of
    its four sides, reaching in."""
    W, H = 203, 147  # ragged: the last tile column holds 11 pixels, the last row 3
    cam = make_camera(W, H)
    rng = np.random.default_rng(47)
    pts = []
    for kx in range(0, 14):
        for ky in range(0, 10):
            ox, oy = rng.choice([0.0, -0.5, -1.0, 15.0, 7.3], 2)
            pts.append((16 * kx + ox, 16 * ky + oy))
    n_in = len(pts)
    for k in range(160):  # outside, on each side in turn
        d = rng.uniform(1.0, 40.0)
        side = k % 4
        pts.append([(-d, rng.uniform(0, H)), (W - 1 + d, rng.uniform(0, H)), (rng.uniform(0, W), -d), (rng.uniform(0, W), H - 1 + d)][side])
    pts = np.array(pts)
    P = len(pts)
    sc = _blank(P, 47)
    z = rng.uniform(3.0, 8.0, P)
    sc.means3D[:] = place(cam, pts[:, 0], pts[:, 1], z)
    s = np.exp(rng.normal(1.2, 0.8, (P, 2)))
    s[n_in:] = np.exp(rng.normal(2.6, 0.4, (P - n_in, 2)))
    _set_sigma_px(sc, cam, np.arange(P), s[:, 0], s[:, 1], z)
    sc.rotations[:] = _rot_z(rng.uniform(0, np.pi, P) * (rng.uniform(size=P) < 0.5))
    sc.opacities[:, 0] = np.exp(rng.uniform(np.log(1.0 / 255), 0.0, P)).astype(np.float32)
    return sc, cam


def _boxes(cam, shapes, o=0.1, seed=53, filler=0):
    """One axis-aligned Gaussian per (nx, ny, kx0, ky0): its contribution box covers exactly the tile columns kx0 .. kx0 + nx - 1
    and rows ky0 .. ky0 + ny - 1, with 7.5 px to spare on every side (the centre sits in the middle of the rectangle, the half
    width is 8 n - 8 px, or 5 px for a single tile).  o = 0.1 keeps the box (2.56 sigma) inside the 3-sigma rectangle."""
    P = len(shapes) + filler
    sc = _blank(P, seed)
    rng = np.random.default_rng(seed)
    W, H = cam.image_width, cam.image_height
    sc.means3D[:] = place(cam, rng.uniform(0, W, P), rng.uniform(0, H, P), rng.uniform(5.5, 8.0, P))
    sf = np.exp(rng.normal(1.5, 0.5, (P, 2)))
    _set_sigma_px(sc, cam, np.arange(P), sf[:, 0], sf[:, 1], sc.means3D[:, 2] + 5.0)
    sc.opacities[:, 0] = rng.uniform(0.05, 0.9, P).astype(np.float32)
    ids = rng.permutation(P)[:len(shapes)]
    tau = tau_of(float(np.float32(o)))
    for i, (nx, ny, kx0, ky0) in zip(ids, shapes):
        hx, hy = max(8.0 * nx - 8.0, 5.0), max(8.0 * ny - 8.0, 5.0)
        z = 3.0 + 0.01 * (int(i) % 97)
        sc.means3D[i] = place(cam, 16.0 * kx0 + 8.0 * nx - 0.5, 16.0 * ky0 + 8.0 * ny - 0.5, z)
        sx, sy = (math.sqrt(max(h * h / (2.0 * tau) - 0.3, 1e-6)) for h in (hx, hy))
        sc.scales[i] = 1e-4
        _set_sigma_px(sc, cam, i, sx, sy, z)
        sc.opacities[i, 0] = o
    return sc, cam


def rect_counts_small():
    """Box rectangles of exactly 63, 64 and 65 tiles, of 128, 129 and more, on a grid of 1125 tiles (at most 2048: the big
    rectangles go through the queue of emit_big_k)."""
    cam = make_camera(720, 400)  # 45 x 25 tiles
    shapes = [(7, 9, 1, 2), (9, 7, 20, 3), (8, 8, 3, 10), (4, 16, 30, 4), (16, 4, 10, 20),
              (5, 13, 12, 6), (13, 5, 25, 15), (32, 2, 6, 1), (21, 3, 2, 21), (3, 21, 36, 2),
              (8, 16, 15, 5), (16, 8, 22, 12), (43, 3, 1, 11), (12, 12, 28, 6), (10, 13, 4, 8),
              (13, 10, 18, 1), (1, 1, 44, 24), (1, 2, 0, 23), (2, 1, 43, 0), (11, 12, 30, 12), (16, 9, 8, 14)]
    shapes = [s for s in shapes if s[0] + s[2] <= 45 and s[1] + s[3] <= 25]
    return _boxes(cam, shapes, filler=300)


def rect_counts_large():
    """The same rectangle sizes on a grid of 3600 tiles (more than 2048: emit's in-kernel loop writes the big rectangles), and
    single-row rectangles of exactly 64 columns (the mask's `c1 - c0 >= 64` case) and of more."""
    cam = make_camera(1280, 720)  # 80 x 45 tiles
    shapes = [(7, 9, 1, 2), (9, 7, 20, 3), (8, 8, 3, 10), (4, 16, 30, 4), (16, 4, 10, 20), (2, 32, 70, 5), (5, 13, 12, 26),
              (13, 5, 45, 35), (64, 1, 3, 40), (64, 1, 16, 1), (1, 45, 79, 0), (65, 1, 10, 43), (72, 1, 4, 30),
              (8, 16, 50, 5), (16, 8, 52, 22), (43, 3, 30, 31), (3, 43, 0, 1), (12, 12, 60, 6), (10, 13, 34, 8), (13, 10, 18, 11),
              (32, 4, 40, 0), (4, 32, 75, 10), (20, 20, 55, 24), (1, 1, 0, 44), (63, 1, 2, 25), (1, 44, 40, 0)]
    return _boxes(cam, shapes, filler=400, seed=59)


def depth_ties():
    """Groups of well over 65 Gaussians at bit-equal depth, at non-adjacent ids (what cloning a Gaussian produces): the order
    inside a tile's list is then the stable one, by id."""
    W, H = 160, 120
    cam = make_camera(W, H)
    P = 900
    sc = _blank(P, 61, S=7)
    rng = np.random.default_rng(61)
    z = rng.uniform(3.0, 8.0, P)
    ids = np.arange(P)
    z[ids % 3 == 0] = 4.25
    z[ids % 5 == 1] = 6.5
    z[(ids % 7 == 3) & (ids % 3 != 0) & (ids % 5 != 1)] = np.float32(5.1)
    sc.means3D[:] = place(cam, rng.uniform(0, W, P), rng.uniform(0, H, P), z)
    s = np.exp(rng.normal(2.0, 0.6, (P, 2)))
    _set_sigma_px(sc, cam, ids, s[:, 0], s[:, 1], z)
    sc.rotations[:] = _rot_z(rng.uniform(0, np.pi, P))
    sc.opacities[:, 0] = rng.uniform(0.02, 1.0, P).astype(np.float32)
    dup = rng.choice(P // 2, 60, replace=False)  # exact clones, far apart in id
    for name in ("means3D", "scales", "rotations", "opacities", "shs", "semantics"):
        getattr(sc, name)[P - 60:] = getattr(sc, name)[dup]
    return sc, cam


LISTED_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def listed_count(V):
    """Exactly V listed Gaussians, interleaved with Gaussians that are listed nowhere: below 1/255 (visible, radius > 0),
    behind the camera, far outside the image."""
    W, H = 176, 112
    cam = make_camera(W, H)
    P = 2 * V + 5
    sc = _blank(P, 67 + V)
    rng = np.random.default_rng(67 + V)
    z = rng.uniform(3.0, 8.0, P)
    sc.means3D[:] = place(cam, rng.uniform(8, W - 8, P), rng.uniform(8, H - 8, P), z)
    s = np.exp(rng.normal(1.3, 0.5, (P, 2))) + 1.0
    _set_sigma_px(sc, cam, np.arange(P), s[:, 0], s[:, 1], z)
    sc.opacities[:, 0] = rng.uniform(0.2, 0.95, P).astype(np.float32)
    listed = np.zeros(P, bool)
    listed[rng.permutation(P)[:V]] = True
    un = np.nonzero(~listed)[0]
    kind = np.arange(un.size) % 3
    sc.opacities[un[kind == 0], 0] = np.float32(0.9) * INV255           # visible, never reaches 1/255
    sc.means3D[un[kind == 1], 2] = -5.5                                  # behind the camera
    sc.means3D[un[kind == 2], 0] += 60.0                                 # far outside the frustum
    return sc, cam


def sweep_config(k):
    rng = np.random.default_rng(7000 + k)
    P = int(rng.choice([40, 150, 400, 900, 1600, 2500]))
    W, H = int(rng.integers(17, 420)), int(rng.integers(17, 310))
    S = int(rng.choice([1, 3, 4, 8, 16]))
    mu = float(rng.uniform(-4.6, -3.0))
    return P, W, H, S, mu


def sweep(k):
    """Heavy-tailed anisotropic scales (the clustered generator), log-uniform opacity over [0.9 / 255, 1], ragged images."""
    P, W, H, S, mu = sweep_config(k)
    # Every fourth configuration is a NEEDLE configuration: the clustered generator as it is (8 % needles, aspect ratios up to
    # 300 : 1, axes up to 3 scene units).  The other three cap the aspect ratio at 10 : 1 and the longest axis at about 20 px:
    # rectangles of more than 64 tiles, where only the box is claimed and its corners are nobody's (the free band), are the
    # business of the hand-built cases and of every fourth draw.
    needle = k % 4 == 0
    max_scale = 3.0 if needle else 20.0 * 5.0 / (W / (2.0 * math.tan(0.5)))
    sc = make_clustered_scene(P, S=S, sh_degree=int(k % 3), seed=7000 + k, extent=(2.0, 1.5, 1.0), log_scale_mean=mu,
                              n_clusters=6, needle_frac=0.08 if needle else 0.0, giant_frac=0.0, max_scale=max_scale,
                              max_aspect=300.0 if needle else 10.0)
    rng = np.random.default_rng(17000 + k)
    sc.opacities[:, 0] = np.exp(rng.uniform(np.log(0.9 / 255), 0.0, P)).astype(np.float32)
    sc.opacities[rng.uniform(size=P) < 0.03, 0] = 1.0
    cam = make_camera(W, H, yaw=float(rng.uniform(-0.4, 0.4)), pitch=float(rng.uniform(-0.25, 0.25)))
    return sc, cam


def large_grid(P, S, W, H, mu, deg):
    return make_scene(P, S=S, sh_degree=deg, seed=3, log_scale_mean=mu), make_camera(W, H, yaw=0.1, pitch=-0.05)


N_SWEEP = 40
# Cases built with needles ON PURPOSE.  Between two culling variants every (quadrant, Gaussian) partial row of the backward is
# identical and only the ORDER of one fp32 sum over a Gaussian's rows differs: about 1e-6 relative on the blend-level gradients
# (16 rows per chunk x 2^-24).  The cov2D -> cov3D -> scale / rotation chain amplifies that by the condition number of the
# covariance, about the SQUARE of the aspect ratio: at 10 : 1 it stays a decade under the 1e-3 criterion of
# tests/test_gpu_parity.py::_check_culled, at 300 : 1 it reaches 1e-2 on the needle's own rows (measured: every row beyond 1e-3
# belongs to a Gaussian of aspect 115 or more, rows of aspect <= 30 agree to 2e-5, and the oracle is as far from either
# variant as they are from each other; docs/MEASUREMENT_LOG.md).  On these cases the geometry gradients of the needles measure
# conditioning, not the lists; everything the blend produces (outputs, opacity, semantics, colour, mean2D) is held as elsewhere.
NEEDLE_CASES = ("needles", "needles_wide") + tuple(f"sweep_{k:02d}" for k in range(0, N_SWEEP, 4))
NEEDLE_ASPECT = 30.0  # rows of a needle case that are still held to 1e-3: Gaussians whose scale aspect ratio is at most this

CASES = {
    "opacity_edges": opacity_edges,
    "needles": needles,
    "needles_wide": lambda: needles(seed=44, W=1000, H=90, n_far=30, n_mid=600),
    "tile_borders": tile_borders,
    "rect_counts_small": rect_counts_small,
    "rect_counts_large": rect_counts_large,
    "depth_ties": depth_ties,
}
CASES.update({f"listed_{V}": (lambda V=V: listed_count(V)) for V in LISTED_COUNTS})
CASES.update({f"sweep_{k:02d}": (lambda k=k: sweep(k)) for k in range(N_SWEEP)})
# the three large grids of tests/test_gpu_parity.py::CASES: the counting emit (8 832 tiles), the non-counting emit (12 288) and
# the separate tile_ranges_hist_k / ranges_k passes (32 400)
CASES.update({
    "grid_2048x1104": lambda: large_grid(6000, 4, 2048, 1104, -4.2, 1),
    "grid_2048x1536": lambda: large_grid(6000, 4, 2048, 1536, -4.2, 1),
    "grid_3840x2160": lambda: large_grid(6000, 4, 3840, 2160, -4.8, 1),
})
BG = np.array([0.2, 0.1, 0.4], np.float32)


def depth_cut_scene():
    """The depth-cut part's scene: well conditioned (make_scene), 50 k Gaussians at 400 x 300."""
    return make_scene(50_000, S=16, sh_degree=3, seed=9, log_scale_mean=-3.5), make_camera(400, 300, yaw=-0.15, pitch=0.05)
