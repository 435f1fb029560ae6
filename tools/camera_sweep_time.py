"""Times the relevant-camera precompute (gui/main.py:407-478) on the 1 M-Gaussian headline scene with 64 orbit cameras at
512 x 512, and writes profiles/camera_sweep.json.

    (a) reference: the reference's loop restated on this package -- render_gui, the fused decode, then per camera
        cos_sim.any(), torch.count_nonzero, Python max() on tensors, mask.float().cpu().numpy(), a host dilation by
        scipy.ndimage.binary_dilation(ones((3,3)), iterations=5) (cv2's stand-in) >= 0.5, torch.from_numpy(...).to(device)
        and a .item() of the count; then the removal loop.
    (b) sweep: semantic.relevant_cameras (one batched dilation on the device, one read-back).
Both take a host clock around a synchronisation, median of --reps after one warm-up, in the same process.  Device events
time the renders + decodes alone and the mask stage alone (pack of every view, the batched dilation, the filter and the
unpack of every view, on maps rendered beforehand), so the mask stage's share of (b) is measured, not inferred.  The
per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of --only-sweep, merged in with
--kernel-stats.

    python tools/camera_sweep_time.py [--out profiles/camera_sweep.json] [--reps 3] [--views 64] [--size 512]
    python tools/camera_sweep_time.py --only-sweep --reps 2            (the driver of the rocprofv3 run)
    python tools/camera_sweep_time.py --kernel-stats <kernel_stats.csv>  (adds kernel_split to --out, no GPU)
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def setup(views, size, dev):
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import HEADLINE, make_orbit_cameras, make_scene
    from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, code_scores, svm_score_fn
    sc = make_scene(HEADLINE["P"], S=HEADLINE["S"], sh_degree=3, seed=0, extent=HEADLINE["extent"],
                    log_scale_mean=HEADLINE["log_scale_mean"], log_scale_std=HEADLINE["log_scale_std"])
    pc = GaussianSet.from_scene(sc, dev)
    cams = [TorchCamera(c, dev) for c in make_orbit_cameras(size, size, n=views)]
    torch.manual_seed(0)
    n_codes = 300
    mlp = SemanticModel(dim_in=HEADLINE["S"], dim_out=n_codes, num_layer=1, use_bias=True, device=dev)
    lut = torch.randn(n_codes, 256, device=dev)
    svm = LinearSVM().to(dev)
    score_fn = svm_score_fn(svm)
    # the prompt: a threshold that keeps the top fifth of the codes, so a view's mask is a part of it, not all of it
    thresh = float(torch.quantile(code_scores(lut, score_fn), 0.8))
    return pc, cams, mlp, lut, score_fn, thresh


def reference_loop(cams, pc, mlp, lut, score_fn, thresh, bg, size):
    """gui/main.py:407-478 with the host dilation; returns (kept indices, seconds spent in the host mask round trips)."""
    from scipy import ndimage

    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import compute_similarity
    host_s = 0.0
    pc.set_semantic_masks()
    max_relative_number = 0
    relative = []
    kernel = np.ones((3, 3), bool)
    for ind, cam in enumerate(cams):
        out = render_gui(cam, pc, bg)
        cos_sim = compute_similarity(out["semantics"], mlp, lut, score_fn, thresh)
        if cos_sim.any():
            n = torch.count_nonzero(cos_sim)
            max_relative_number = max(max_relative_number, n)
            mask = (cos_sim > 0).reshape(size, size, -1).permute(2, 0, 1)
            t0 = time.perf_counter()
            m = mask.detach().to(dtype=torch.float32).cpu().numpy().squeeze(0)
            d = ndimage.binary_dilation(m, kernel, iterations=5, border_value=0).astype(np.float32) >= 0.5
            dilated = torch.from_numpy(d).unsqueeze(0).to(mask.device)
            n_item = n.item()
            host_s += time.perf_counter() - t0
            relative.append((ind, n, mask, dilated, n_item))
    i = 0
    while i < len(relative):
        if relative[i][1] < max_relative_number * 0.1:
            relative.remove(relative[i])
        else:
            i += 1
    pc.set_semantic_masks(None)
    return [r[0] for r in relative], host_s


def host_ms(fn, reps):
    ts, res = [], None
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if r:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), res


def event_ms(fn, reps):
    ts = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def measure(args, dev):
    from goi_hyperplane_amd import _lib, masks
    from goi_hyperplane_amd.render import render_gui
    from goi_hyperplane_amd.semantic import compute_similarity, relevant_cameras, relevant_keep
    _lib.load()
    V, S = args.views, args.size
    pc, cams, mlp, lut, score_fn, thresh = setup(V, S, dev)
    bg = torch.zeros(3, device=dev)
    sweep = lambda: relevant_cameras(cams, pc, mlp, lut, score_fn, thresh, bg)  # noqa: E731
    if args.only_sweep:
        for _ in range(args.reps + 1):
            sweep()
        torch.cuda.synchronize()
        return None
    sweep_ms, res = host_ms(sweep, args.reps)
    ref_ms, (ref_index, _) = host_ms(lambda: reference_loop(cams, pc, mlp, lut, score_fn, thresh, bg, S), args.reps)
    host_parts = [reference_loop(cams, pc, mlp, lut, score_fn, thresh, bg, S)[1] * 1e3 for _ in range(args.reps)]
    assert ref_index == res.index, (ref_index, res.index)

    sims = []

    def render_decode():
        sims.clear()
        for cam in cams:
            sims.append(compute_similarity(render_gui(cam, pc, bg)["semantics"], mlp, lut, score_fn, thresh).reshape(S, S))

    render_ms = event_ms(render_decode, args.reps)
    packed = torch.empty((V, S, masks.words(S)), dtype=torch.int64, device=dev)
    counts = torch.zeros((V, 2), dtype=torch.int64, device=dev)
    every = torch.arange(V, device=dev)

    def mask_stage():
        counts.zero_()
        for v in range(V):
            masks.pack_into(sims[v], packed, counts, v)
        dilated = masks.dilate_packed(packed, S, 5)
        relevant_keep(counts[:, 0])
        masks.unpack(packed, S, every)
        masks.unpack(dilated, S, every)

    mask_ms = event_ms(mask_stage, args.reps)
    dil_ms = event_ms(lambda: masks.dilate_packed(packed, S, 5), args.reps)
    c0, k = res.counts.cpu(), len(res.index)
    return {
        "what": "relevant-camera precompute (gui/main.py:407-478): restated reference loop with a host dilation vs "
                "semantic.relevant_cameras; tools/camera_sweep_time.py",
        "device": torch.cuda.get_device_name(dev), "scene": "headline (1 M Gaussians), make_orbit_cameras",
        "views": V, "W": S, "H": S, "reps": args.reps, "thresh": round(thresh, 6), "kept": k,
        "count_nonzero_min_median_max": [int(c0.min()), int(c0.median()), int(c0.max())],
        "reference_loop": {"ms_total": round(ref_ms, 2), "ms_per_camera": round(ref_ms / V, 3),
                           "host_mask_round_trips_ms_total": round(statistics.median(host_parts), 2)},
        "relevant_cameras": {"ms_total": round(sweep_ms, 2), "ms_per_camera": round(sweep_ms / V, 3)},
        "speedup": round(ref_ms / sweep_ms, 2),
        "device_events": {"render_decode_ms_total": round(render_ms, 3),
                          "mask_stage_ms_total": round(mask_ms, 4), "mask_stage_us_per_view": round(mask_ms * 1e3 / V, 2),
                          "mask_stage_share_of_sweep": round(mask_ms / sweep_ms, 4),
                          "batched_dilation_ms": round(dil_ms, 4),
                          "mask_stage_note": "pack of every view, one dilation, the filter, unpack of every view "
                                             "(the sweep unpacks the kept views only)"},
    }


def kernel_split(csv_path):
    """Rows of a rocprofv3 --stats kernel_stats.csv: the mask kernels and the ten largest."""
    with open(csv_path) as fh:
        rows = list(csv.DictReader(fh))
    out = [{"kernel": r["Name"][:120], "calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 4),
            "avg_us": round(float(r["AverageNs"]) / 1e3, 3), "percent": round(float(r["Percentage"]), 3)} for r in rows]
    out.sort(key=lambda r: -r["total_ms"])
    return {"source": "rocprofv3 --kernel-trace --stats of tools/camera_sweep_time.py --only-sweep",
            "mask_kernels": [r for r in out if "mask_" in r["kernel"]], "top10": out[:10]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_sweep.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--only-sweep", action="store_true", help="relevant_cameras only (for the rocprofv3 kernel split)")
    ap.add_argument("--kernel-stats", help="merge a rocprofv3 kernel_stats.csv into --out as kernel_split (no GPU)")
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as fh:
            doc = json.load(fh)
        doc["kernel_split"] = kernel_split(args.kernel_stats)
    else:
        doc = measure(args, torch.device("cuda:0"))
        if doc is None:
            return
    print(json.dumps(doc, indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
