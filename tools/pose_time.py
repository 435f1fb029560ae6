"""Times the pose gradient of a selection (goi_hyperplane_amd.pose.gradient, csrc/pose.hip) against the same
reduction restated in torch on the same device, and writes profiles/pose_gradient.json.

    workload   1 M Gaussians, SH degree 3 (M = 16), seeded gradients in the four .grad tensors; 10 %, 50 % and 100 % selected at
               random
    kernel     pose.gradient(g, sel, pivot="centroid"): two launches for the centroid, two for the reduction, no host
               synchronisation
    torch      boolean-mask indexing of the eight tensors, the centroid by mean, cross products, the quaternion term written out,
               one einsum per axis against the dense SH generators, float64 sums over the rows

Both paths are warmed and then ALTERNATE in the same process: --reps windows each, a window being two device events around one
call and ending in a synchronise.  Recorded per path: median, quartiles, extremes and the medians of the two halves of the
windows.  The kernel path is also timed with 8 calls queued per window (the host prepares the next call while the device runs the
last one).  The kernel's algorithmic bytes -- 428 per selected row (12 + 12 + 16 + 16 + 12 + 180 + 180), the selection bytes
twice, the selected positions once more for the centroid -- over that time give the achieved bytes per second, stated against the
6.29 TB/s streaming figure of this device.

For information, not a gate: the analytic directional derivative dL/dtau . u of a photometric loss through the renderer against
central differences (L(T(+h u)) - L(T(-h u))) / 2h at two step sizes, for a selection (edit.transform) and for the camera
(edit.transform_camera).  The rasterizer's alpha and radius cut-offs make the loss only piecewise smooth and its arithmetic is
fp32, so the two agree to a few digits at best.  Needs a GPU.

    python tools/pose_time.py [--out profiles/pose_gradient.json] [--reps 30]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from edit_time import STREAM_TBS, alternate  # noqa: E402

FRACTIONS = (0.1, 0.5, 1.0)
QUEUED = 8
ROW_BYTES = 428


def scene_model(sc, dev):
    """A reference-style model (raw parameters) holding the scene `sc`."""
    from tests import densify_reference as dref
    t = lambda a: torch.nn.Parameter(torch.tensor(a, dtype=torch.float32, device=dev).contiguous())  # noqa: E731
    m = dref.Model()
    m._xyz, m._scaling, m._rotation = t(sc.means3D), t(np.log(sc.scales)), t(sc.rotations)
    m._opacity = t(np.log(sc.opacities / (1 - sc.opacities)))
    m._features_dc, m._features_rest, m._semantics = t(sc.shs[:, :1]), t(sc.shs[:, 1:]), t(sc.semantics)
    return m


def build_model(P, dev):
    """The headline scene as a model, with seeded gradients in the four tensors a similarity moves."""
    from goi_hyperplane_amd import pose
    from goi_hyperplane_amd.scene import HEADLINE, make_scene
    sc = make_scene(P, S=HEADLINE["S"], sh_degree=3, seed=0, extent=HEADLINE["extent"], log_scale_mean=HEADLINE["log_scale_mean"],
                    log_scale_std=HEADLINE["log_scale_std"])
    m = scene_model(sc, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    for attr in pose.GRADS:
        p = getattr(m, attr)
        p.grad = 1e-3 * torch.randn(p.shape, device=dev, generator=gen)
    return m


class TorchPose:
    """The reduction restated in torch: the generators on the device once, then mask indexing and a dozen passes per call."""

    def __init__(self, dev):
        from goi_hyperplane_amd import pose
        self.G = torch.tensor(pose.sh_generators(3)[:, 1:, 1:], dtype=torch.float32, device=dev)

    @torch.no_grad()
    def __call__(self, g, sel):
        x, gx = g._xyz[sel], g._xyz.grad[sel]
        d = x - x.mean(dim=0)
        r, gr = g._rotation[sel], g._rotation.grad[sel]
        w, v, gw, gv = r[:, :1], r[:, 1:], gr[:, :1], gr[:, 1:]
        c, gc = g._features_rest[sel], g._features_rest.grad[sel]
        colour = torch.stack([torch.einsum("nic,ij,njc->n", gc, self.G[k], c) for k in range(3)], dim=1)
        omega = torch.linalg.cross(d, gx).double().sum(0) + (0.5 * (w * gv - gw * v + torch.linalg.cross(v, gv))).double().sum(0) \
            + colour.double().sum(0)
        t = gx.double().sum(0)
        sigma = (gx * d).sum(1).double().sum() + g._scaling.grad[sel].sum(1).double().sum()
        return torch.cat([omega, t, sigma.reshape(1)])


def check_paths_agree(dev):
    """one call both ways on a small model: the same seven numbers to the fp32 rounding of the pieces and of torch's centroid"""
    from goi_hyperplane_amd import pose
    g = build_model(20000, dev)
    sel = torch.rand(20000, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) < 0.5
    out = pose.gradient(g, sel, pivot="centroid")
    a = torch.cat([out["rotation"], out["translation"], out["log_scale"].reshape(1)])
    b = TorchPose(dev)(g, sel)
    worst = float((a - b).abs().max() / a.abs().max())  # relative to the largest component
    assert worst < 1e-4, (a, b)
    return worst


def algorithmic_bytes(P, n_sel):
    """the seven rows of every selected Gaussian once, the selection bytes for the bounds and for the reduction, the selected
    positions once more for the centroid"""
    return n_sel * (ROW_BYTES + 12) + 2 * P


# ---- the directional derivative through the renderer (reported, not gated) ----------------------------------------------------
def derivative_check(dev):
    from goi_hyperplane_amd import edit, pose
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera, make_scene
    P = 20000
    sc = make_scene(P, S=4, seed=2, log_scale_mean=-3.0)
    cam = make_camera(256, 256, yaw=0.3, pitch=-0.2)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = PipelineParams()
    with torch.no_grad():
        target = render(TorchCamera(make_camera(256, 256, yaw=0.33, pitch=-0.18), dev), scene_model(sc, dev), pipe, bg)["render"]

    def loss_of(m, camera, wanted):
        return ((render(TorchCamera(camera, dev), m, pipe, bg)["render"].double() - wanted.double()) ** 2).mean()

    # the selection: a ball of Gaussians displaced from where the target (the unedited model, same camera) shows it
    sel = torch.zeros(P, dtype=torch.bool, device=dev)
    sel[torch.tensor(np.flatnonzero(np.linalg.norm(sc.means3D - np.array([0.3, 0.1, 0.0], np.float32), axis=1) < 0.7), device=dev)] = True
    with torch.no_grad():
        placed = render(TorchCamera(cam, dev), scene_model(sc, dev), pipe, bg)["render"]
    displaced = dict(rotation=pose.twist_rotation(math.radians(2.0) * np.array([0.0, 0.6, 0.8])), translation=(0.04, -0.03, 0.02),
                     pivot="centroid")

    def displaced_model():
        moved = scene_model(sc, dev)
        edit.transform(moved, sel, **displaced)
        return moved

    m = displaced_model()
    loss_of(m, cam, placed).backward()
    pivot = edit.selection_bounds(m._xyz.detach(), sel)["centroid"].cpu().numpy().astype(np.float64)
    res = pose.gradient(m, sel, pivot=pivot)
    grad = torch.cat([res["rotation"], res["translation"], res["log_scale"].reshape(1)]).cpu().numpy()
    # the camera: the whole model against a render from a nearby camera, twisted about the camera's centre
    whole = scene_model(sc, dev)
    loss_of(whole, cam, target).backward()
    centre = np.asarray(cam.camera_center, dtype=np.float64)
    cres = pose.camera_gradient(whole, pivot=centre)
    cgrad = torch.cat([cres["rotation"], cres["translation"]]).cpu().numpy()
    rng = np.random.default_rng(0)
    u = rng.normal(size=7)
    u /= np.linalg.norm(u)
    uc = rng.normal(size=6)
    uc /= np.linalg.norm(uc)
    rows = {"selected": int(sel.sum()), "P": P, "image": "256 x 256",
            "selection": {"loss": "mean squared error of the model with the selection displaced (2 degrees, 0.054) against its own "
                                  "undisplaced render", "gradient": grad.tolist(), "direction": u.tolist(),
                          "analytic": float(grad @ u), "central_differences": {}},
            "camera": {"loss": "mean squared error against a render from a nearby camera (yaw + 0.03, pitch + 0.02)",
                       "gradient": cgrad.tolist(), "direction": uc.tolist(), "analytic": float(cgrad @ uc), "central_differences": {}}}
    for h in (1e-3, 1e-4):
        vals = []
        for sign in (1.0, -1.0):
            moved = displaced_model()
            tau = sign * h * u
            edit.transform(moved, sel, rotation=pose.twist_rotation(tau[:3]), translation=tau[3:6], scale=math.exp(tau[6]), pivot=pivot)
            with torch.no_grad():
                vals.append(float(loss_of(moved, cam, placed)))
        rows["selection"]["central_differences"][f"h={h:g}"] = (vals[0] - vals[1]) / (2 * h)
        vals = []
        for sign in (1.0, -1.0):
            tau = sign * h * uc
            moved_cam = edit.transform_camera(cam, rotation=pose.twist_rotation(tau[:3]), translation=tau[3:6], pivot=centre)
            with torch.no_grad():
                vals.append(float(loss_of(whole, moved_cam, target)))
        rows["camera"]["central_differences"][f"h={h:g}"] = (vals[0] - vals[1]) / (2 * h)
    for k in ("selection", "camera"):
        a = rows[k]["analytic"]
        rows[k]["relative_difference"] = {h: abs(v - a) / max(abs(a), 1e-300) for h, v in rows[k]["central_differences"].items()}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_gradient.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--P", type=int, default=1_000_000)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps must be at least 30")
    assert torch.cuda.is_available(), "tools/pose_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _lib, pose
    _lib.load()
    agree = check_paths_agree(dev)
    derivative = derivative_check(dev)
    print(json.dumps(derivative), flush=True)
    P = args.P
    g = build_model(P, dev)
    restated = TorchPose(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for frac in FRACTIONS:
        sel = torch.rand(P, device=dev, generator=gen) < frac if frac < 1.0 else torch.ones(P, dtype=torch.bool, device=dev)
        n_sel = int(sel.sum())
        kernel = lambda w: pose.gradient(g, sel, pivot="centroid")  # noqa: E731
        torch_path = lambda w: restated(g, sel)  # noqa: E731
        for w in range(4):
            kernel(w)
            torch_path(w)
        calls = alternate({"torch": torch_path, "kernel": kernel}, args.reps)
        queued = alternate({"kernel": lambda w: [kernel(w) for _ in range(QUEUED)]}, args.reps)["kernel"]
        per_call = queued["median_ms"] / QUEUED
        nbytes = algorithmic_bytes(P, n_sel)
        tbs = nbytes / (per_call * 1e-3) / 1e12
        row = {"selected_fraction": frac, "selected": n_sel, "call": calls,
               "speedup_median": round(calls["torch"]["median_ms"] / calls["kernel"]["median_ms"], 2),
               "kernel_quartiles_below_torch": bool(calls["kernel"]["q3_ms"] < calls["torch"]["q1_ms"]),
               "kernel_queued": dict(queued, calls_per_window=QUEUED, ms_per_call=round(per_call, 4)),
               "kernel_algorithmic_bytes": nbytes, "kernel_tb_per_s": round(tbs, 3),
               "fraction_of_streaming_6p29_tb_per_s": round(tbs / STREAM_TBS, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = {"what": "pose.gradient (dL/d(omega, t, sigma) of a selection from the .grad tensors of one backward; centroid pivot derived "
                   "on the device) against the same reduction restated in torch; tools/pose_time.py",
           "device": torch.cuda.get_device_name(dev), "P": P, "sh_degree": 3, "paths_agree_max_abs_over_largest_component": agree,
           "streaming_tb_per_s": STREAM_TBS, "row_bytes": ROW_BYTES,
           "statistic": "two device events around one call, the window ending in a synchronise; the two paths alternate in one process "
                        "after four warm-up rounds of both; median, quartiles, extremes and the medians of the two halves; "
                        "kernel_queued: the same windows around 8 calls in a row, kernel_tb_per_s from its time per call",
           "rows": rows,
           "directional_derivative_through_the_renderer": dict(derivative, note="for information, not a gate: the loss is only "
                                                               "piecewise smooth (alpha and radius cut-offs) and rendered in fp32")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
