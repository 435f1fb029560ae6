"""Times a render of PART of the model two ways and writes profiles/selection.json: the index-select path (render(...,
gaussian_mask=m): the reference's gui/gs_renderer.py:315-321, a boolean index-select of every per-Gaussian tensor in front of
the rasterizer) against the in-place path (in_place=True: the mask goes to the rasterizer as a selection).

    (a) viewer frame: the 1 M-Gaussian headline scene at 1600 x 1056, SH degree 3, S = 16, a random 50 % kept, render_gui under
        torch.no_grad() -- what the viewer's 3D seg / del modes display;
    (b) edit step: BASELINE config 5 as tests/test_gpu_configs.py states it -- 6 M Gaussians, 512 x 512, a random 60 % kept,
        the masked-MSE loss, forward + backward with every parameter trainable.

For each workload both paths are warmed, the equalities of tests/test_gpu_selection.py's forward test are asserted (the four
maps and num_rendered equal, radii[m] the subset's radii, radii[~m] zero), and then the two paths ALTERNATE in the same process:
--reps windows each, a window being two device events around one frame / step and ending in a synchronise.  Recorded per path:
the median, the quartiles, the extremes and the medians of the first and second half of the windows (how far the same path's
median moves between two runs in one call: what a difference between the paths has to be compared with), and
torch.cuda.max_memory_allocated of one further window, measured from a reset after the previous window's gradients have been
dropped (model, workspaces kept by the library and the allocator's state are in the figure for both paths alike;
peak_above_before_bytes is what the window itself added).  Needs a GPU.

    python tools/selection_time.py [--out profiles/selection.json] [--reps 30]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

MAPS = ("image", "semantics", "depth", "alpha")


def build(P, W, H, seed, dev, yaw=0.0, pitch=0.0, orbit=False):
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import HEADLINE, make_camera, make_orbit_cameras, make_scene
    sc = make_scene(P, S=HEADLINE["S"], sh_degree=3, seed=seed, extent=HEADLINE["extent"],
                    log_scale_mean=HEADLINE["log_scale_mean"], log_scale_std=HEADLINE["log_scale_std"])
    pc = GaussianSet.from_scene(sc, dev)
    cam = make_orbit_cameras(W, H, n=8)[0] if orbit else make_camera(W, H, fovx=HEADLINE["fovx"], yaw=yaw, pitch=pitch)
    return pc, TorchCamera(cam, dev)


def check_equal(a, b, keep):
    """a: the in-place frame, b: the index-select frame (render_gui dictionaries, counts read)"""
    for k in MAPS:
        assert torch.equal(a[0][k], b[0][k]), f"{k}: the in-place frame differs from the index-select frame"
    assert a[1] == b[1], (a[1], b[1])
    assert torch.equal(a[0]["radii"][keep], b[0]["radii"]) and not a[0]["radii"][~keep].any()


def spread(ts):
    q = statistics.quantiles(ts, n=4)
    half = len(ts) // 2
    return {"median_ms": round(statistics.median(ts), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4),
            "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "median_first_half_ms": round(statistics.median(ts[:half]), 4),
            "median_second_half_ms": round(statistics.median(ts[half:]), 4)}


def alternate(paths, reps, release=lambda: None):
    """paths: {name: callable running one window's work}; release() drops what a window leaves allocated (gradients), so that
    both memory windows start from the same state.  -> {name: spread + peak memory}"""
    times = {n: [] for n in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    out = {}
    for name, fn in paths.items():
        release()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak = int(torch.cuda.max_memory_allocated())
        out[name] = dict(spread(times[name]), windows=reps, max_memory_allocated_bytes=peak,
                         memory_allocated_before_bytes=int(base), peak_above_before_bytes=peak - int(base))
    release()
    return out


def viewer_frame(dev, reps):
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.scene import HEADLINE
    P, W, H = HEADLINE["P"], 1600, 1056
    pc, cam = build(P, W, H, 0, dev, orbit=True)
    bg = torch.zeros(3, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    keep = torch.rand(P, device=dev, generator=g) < 0.5

    def frame(in_place):
        with torch.no_grad():
            out = render_gui(cam, pc, bg, gaussian_mask=keep, in_place=in_place)
        return out, int(rasterizer.last_num_rendered())

    for _ in range(3):
        a, b = frame(True), frame(False)
    check_equal(a, b, keep)
    n = a[1]
    del a, b
    res = alternate({"index_select": lambda: frame(False), "in_place": lambda: frame(True)}, reps)
    return {"workload": "viewer frame", "P": P, "W": W, "H": H, "sh_degree": 3, "S": HEADLINE["S"], "kept": round(float(keep.float().mean()), 4),
            "grad": False, "num_rendered": n, "equalities_asserted": True, "paths": res}


def edit_step(dev, reps):
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.scene import HEADLINE
    P, R = 6_000_000, 512
    pc, cam = build(P, R, R, 5, dev, yaw=0.08, pitch=-0.03)
    white = torch.ones(3, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    keep = torch.rand(P, device=dev, generator=g) < 0.6
    target = torch.rand((3, R, R), device=dev, generator=g)
    yy, xx = torch.meshgrid(torch.arange(R, device=dev), torch.arange(R, device=dev), indexing="ij")
    region = (((xx - 280) ** 2 + (yy - 230) ** 2) < 170 ** 2).float()[None]

    def step(in_place):
        for p in pc.parameters():
            p.grad = None
        out = render_gui(cam, pc, white, gaussian_mask=keep, in_place=in_place)
        (((out["image"] - target) ** 2) * region).sum().backward()
        return out

    def frame(in_place):
        out = step(in_place)
        n = int(rasterizer.last_num_rendered())
        return {k: v.detach() for k, v in out.items() if k != "viewspace_points"}, n, {k: p.grad.clone() for k, p in pc.named_parameters()}

    for _ in range(3):
        a, b = frame(True), frame(False)
    check_equal(a, b, keep)
    grads_equal = {k: bool(torch.equal(a[2][k], b[2][k])) for k in a[2]}
    n = a[1]
    del a, b

    def release():
        for p in pc.parameters():
            p.grad = None

    res = alternate({"index_select": lambda: step(False), "in_place": lambda: step(True)}, reps, release)
    return {"workload": "config-5 edit step (forward + backward, every parameter trainable)", "P": P, "W": R, "H": R, "sh_degree": 3,
            "S": HEADLINE["S"], "kept": round(float(keep.float().mean()), 4), "grad": True, "num_rendered": n,
            "equalities_asserted": True, "gradients_bit_equal": grads_equal, "paths": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selection.json"))
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps must be at least 30")
    assert torch.cuda.is_available(), "tools/selection_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _C, _lib
    _lib.load()
    rows = []
    for fn in (viewer_frame, edit_step):
        rows.append(fn(dev, args.reps))
        print(json.dumps(rows[-1]), flush=True)
        _C.poll_counts(wait=True)
        _C.release_scratch()
        torch.cuda.empty_cache()
    doc = {"what": "a render of part of the model: index-select of every per-Gaussian tensor in front of the rasterizer against the "
                   "selection the rasterizer honours in place (render(..., gaussian_mask=m, in_place=True)); tools/selection_time.py",
           "device": torch.cuda.get_device_name(dev), "binding": _C.binding(), "forward_mode": dict(_C._FWD),
           "statistic": "two device events around one frame / step, the window ending in a synchronise; the two paths alternate in "
                        "one process after three warm-up rounds of both; median, quartiles, extremes and the medians of the two halves "
                        "of the windows; max_memory_allocated of one further window from a reset",
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
