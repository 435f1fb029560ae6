"""Times the contribution replay (goi_raster_contrib_frame, goi_hyperplane_amd.contrib) and writes
profiles/contrib.json.

    (a) the kernel against the forward blend: the headline scene (1 M Gaussians) and the same box at 3 M, 1600 x 1056, first orbit
        camera.  One exact forward; then the replay of that frame in three forms that ALTERNATE in one process -- peak only into a
        zeroed array (every (quadrant, Gaussian) that reached a live pixel issues its atomic unless another quadrant already
        raised the word), peak only into the frame's own result (the skip-load finds every word large enough: no atomic at all),
        and all three outputs -- next to render_fwd_k's stage time for the same frame (goi_raster_profile_collect, mean of
        the same number of forwards) and the frame's blend_stats counters, which bound the atomics: at most word 3 (the pairs
        the forward evaluates), at least word 4 (member pairs: each has a contribution);
    (b) contrib.peak_weights over the 16-camera orbit, the whole call (16 exact forwards, 16 count read-backs, 16 replays);
    (c) what pruning buys: Gaussians with peak <= 0 and with peak < 0.01 over the orbit, the views per second of a plain
        no-grad render of the orbit before and after each prune (the rows are dropped by index-select, which keeps their order
        as densify.prune_points does), the four maps compared by bits at 0 and photometric.psnr per view at 0.01.

A window is two device events around one call and ends in a synchronise; per form the median, quartiles, extremes and the
medians of the two halves of the windows.  Needs a GPU.

    python tools/contrib_time.py [--out profiles/contrib.json] [--reps 30] [--P3 3000000]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

W, H = 1600, 1056
MAPS = ("render", "semantics", "depth", "alpha")


def spread(ts):
    q = statistics.quantiles(ts, n=4)
    half = len(ts) // 2
    return {"median_ms": round(statistics.median(ts), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4),
            "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "median_first_half_ms": round(statistics.median(ts[:half]), 4),
            "median_second_half_ms": round(statistics.median(ts[half:]), 4), "windows": len(ts)}


def alternate(paths, reps, warmup=3):
    times = {n: [] for n in paths}
    for r in range(warmup + reps):
        for name, (prepare, fn) in paths.items():
            prepare()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b))
    return {n: spread(t) for n, t in times.items()}


def model(P, dev):
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import HEADLINE, make_orbit_cameras, make_scene
    sc = make_scene(P, S=HEADLINE["S"], sh_degree=3, seed=0, extent=HEADLINE["extent"], log_scale_mean=HEADLINE["log_scale_mean"],
                    log_scale_std=HEADLINE["log_scale_std"])
    return GaussianSet.from_scene(sc, dev), [TorchCamera(c, dev) for c in make_orbit_cameras(W, H)]


def forward(cam, pc, bg):
    from goi_hyperplane_amd import _C
    d = lambda t: t.detach()  # noqa: E731
    args = (bg, d(pc.get_xyz), torch.Tensor([]), d(pc.get_semantics), d(pc.get_opacity), d(pc.get_scaling), d(pc.get_rotation), 1.0,
            torch.Tensor([]), cam.world_view_transform, cam.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), H, W,
            d(pc.get_features), int(pc.active_sh_degree), cam.camera_center, False, False)
    n, *_maps, geom, binning, img = _C.rasterize_gaussians(*args)
    return int(n), geom, binning, img


def kernel_row(P, dev, reps):
    from goi_hyperplane_amd import _C, _lib, contrib
    pc, cams = model(P, dev)
    bg = torch.zeros(3, device=dev)
    for _ in range(3):
        n, geom, binning, img = forward(cams[0], pc, bg)
    _lib.profile_collect()
    _lib.profile_enable(True)
    for _ in range(reps):
        n, geom, binning, img = forward(cams[0], pc, bg)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ms, calls = _lib.profile_collect()["blend_fwd"]
    stats = _C.blend_stats(P, W, H, n, geom, binning, img)
    own = contrib.frame_buffers(P, W, H, n, geom, binning, img).peak.clone()
    peak = torch.zeros(P, device=dev)
    forms = {
        "peak_from_zero": (peak.zero_, lambda: contrib.frame_buffers(P, W, H, n, geom, binning, img, peak=peak, want_ids=False)),
        "peak_already_there": (lambda: peak.copy_(own), lambda: contrib.frame_buffers(P, W, H, n, geom, binning, img, peak=peak, want_ids=False)),
        "all_three_outputs": (peak.zero_, lambda: contrib.frame_buffers(P, W, H, n, geom, binning, img, peak=peak)),
    }
    res = alternate(forms, reps)
    peak.zero_()
    f = contrib.frame_buffers(P, W, H, n, geom, binning, img, peak=peak)
    assert torch.equal(f.peak, own)
    blend = ms / max(calls, 1)
    row = {"P": P, "W": W, "H": H, "num_rendered": n, "blend_fwd_stage_mean_ms": round(blend, 4), "blend_fwd_calls": calls, "replay": res,
           "ratio_peak_from_zero_to_blend_fwd": round(res["peak_from_zero"]["median_ms"] / blend, 3),
           "ratio_all_three_to_blend_fwd": round(res["all_three_outputs"]["median_ms"] / blend, 3),
           "atomics_upper_bound_forward_pairs": stats["forward_pairs"], "atomics_lower_bound_member_pairs_without_skip": stats["member_pairs"],
           "atomics_with_every_word_already_there": 0, "gaussians_with_peak_above_0": int((own > 0).sum()),
           "pixels_with_a_contributor": int((f.top_id >= 0).sum())}
    del pc, cams, geom, binning, img
    _C.poll_counts(wait=True)
    _C.release_scratch()
    torch.cuda.empty_cache()
    return row


def orbit_rows(dev, reps):
    from goi_hyperplane_amd import contrib, photometric
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, render
    from goi_hyperplane_amd.scene import HEADLINE
    P = HEADLINE["P"]
    pc, cams = model(P, dev)
    bg = torch.zeros(3, device=dev)
    peak = contrib.peak_weights(cams, pc, bg)
    sweep = alternate({"peak_weights_16_cameras": (lambda: None, lambda: contrib.peak_weights(cams, pc, bg))}, max(reps // 3, 8), warmup=1)
    assert torch.equal(contrib.peak_weights(cams[::-1], pc, bg), peak)

    def subset(keep):
        return GaussianSet(*(t[keep].detach().contiguous() for t in (pc._xyz, pc._scaling, pc._rotation, pc._opacity, pc._features, pc._semantics)),
                           pc.active_sh_degree)

    def orbit(m):
        with torch.no_grad():
            return [render(c, m, PipelineParams(), bg) for c in cams]

    def views_per_s(m):
        r = alternate({"orbit": (lambda: None, lambda: orbit(m))}, max(reps // 3, 8), warmup=2)["orbit"]
        return dict(r, views_per_s=round(16e3 / r["median_ms"], 1))

    before = [{k: o[k].clone() for k in MAPS} for o in orbit(pc)]
    out = {"P": P, "cameras": len(cams), "sweep": sweep, "render_before": views_per_s(pc), "prune": {}}
    for thr in (0.0, 0.01):
        mask = (peak <= 0) if thr == 0 else (peak < thr)
        m = subset(~mask)
        after = orbit(m)
        row = {"pruned": int(mask.sum()), "kept": int((~mask).sum()), "render_after": views_per_s(m)}
        if thr == 0:
            row["maps_bit_identical"] = all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for a, b in zip(before, after) for k in MAPS)
        else:
            ps = [float(photometric.psnr(a["render"], b["render"]).mean()) for a, b in zip(before, after)]
            row["psnr_db_min"], row["psnr_db_median"] = round(min(ps), 2), round(statistics.median(ps), 2)
        out["prune"][str(thr)] = row
        del m, after
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--P3", type=int, default=3_000_000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/contrib_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _C, _lib
    from goi_hyperplane_amd.scene import HEADLINE
    _lib.load()
    _C.set_forward_mode(speculative=False)
    doc = {"what": "the contribution replay (peak blend weight per Gaussian, dominant contributor per pixel) against the forward blend, a "
                   "16-camera sweep, and what pruning by peak weight buys; tools/contrib_time.py",
           "device": torch.cuda.get_device_name(dev), "binding": _C.binding(),
           "statistic": "two device events around one call, the window ending in a synchronise; forms alternate in one process after "
                        "warm-up; median, quartiles, extremes, medians of the two halves; blend_fwd: mean stage time of the same number "
                        "of forwards (goi_raster_profile_collect)",
           "kernel": [], "orbit": None}
    for P in (HEADLINE["P"], args.P3):
        doc["kernel"].append(kernel_row(P, dev, args.reps))
        print(json.dumps(doc["kernel"][-1]), flush=True)
    doc["orbit"] = orbit_rows(dev, args.reps)
    print(json.dumps(doc["orbit"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
