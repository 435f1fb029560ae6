"""Times the viewer's frame stage (gui/main.py:549-604 test_step, :387-398 set_clip_mask, :1766-1801 render_video) on one
view of the 1 M-Gaussian headline scene at 1600 x 1056 and 800 x 800, styles HEAT and WHITEN, float32 and uint8, and writes
profiles/display.json.  From one render and one fused decode, resident on the device, in the same process:

    (a) reference: the reference's stage restated -- the image's permute / clamp / .cpu().numpy(), clip_color's torch
        operations on the device with its .cpu().numpy() copies, the numpy blend and clip on the host (and * 255, astype
        uint8 for render_video).  The frame ends in host memory, where the reference's texture or PNG writer takes it.
    (b) display.compose and one device -> host copy of the finished frame into a pinned buffer.
    (c) display.compose alone, by device events.
(a) and (b) take a host clock around a synchronisation; every figure is the median of --reps after one warm-up.  The
per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of --only-compose (one frame size per run),
merged in with --kernel-stats: with the bytes each kernel must move (from the shapes, bytes_moved below) they give a
share of the HBM peak.  The inputs were written by the render and the decode just before, so they may be resident in the
caches: that share is no measurement of HBM traffic.

    python tools/display_time.py [--out profiles/display.json] [--reps 3]
    python tools/display_time.py --only-compose --size 1600x1056          (the driver of a rocprofv3 run)
    python tools/display_time.py --kernel-stats <kernel_stats.csv> --size 1600x1056   (merges into --out, no GPU)
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

SIZES = ((1600, 1056), (800, 800))
STYLES = ("heat", "whiten")
RATIO = 0.6
HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X data sheet
STYLE_CODE = {"heat": 3, "whiten": 2}  # GOI_FRAME_HEAT, GOI_FRAME_WHITEN: the template argument in the kernel names


def bytes_moved(style, uint8, HW, K=256):
    """Bytes the two kernels must read and write for one three-channel view of HW pixels (no normalisation)."""
    out = HW * 3 * (1 if uint8 else 4)
    if style == "heat":
        return {"frame_stats_k": HW * 4 + 12, "frame_compose_k": 3 * HW * 4 + HW * 4 + HW + K * 12 + 12 + out}
    return {"frame_compose_k": 3 * HW * 4 + HW + out}


def setup(W, H, dev):
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera, render_gui
    from goi_hyperplane_amd.scene import HEADLINE, make_orbit_cameras, make_scene
    from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, code_scores, compute_similarity, svm_score_fn
    sc = make_scene(HEADLINE["P"], S=HEADLINE["S"], sh_degree=3, seed=0, extent=HEADLINE["extent"],
                    log_scale_mean=HEADLINE["log_scale_mean"], log_scale_std=HEADLINE["log_scale_std"])
    pc = GaussianSet.from_scene(sc, dev)
    cam = TorchCamera(make_orbit_cameras(W, H, n=8)[0], dev)
    torch.manual_seed(0)
    n_codes = 300
    mlp = SemanticModel(dim_in=HEADLINE["S"], dim_out=n_codes, num_layer=1, use_bias=True, device=dev)
    lut = torch.randn(n_codes, 256, device=dev)
    score_fn = svm_score_fn(LinearSVM().to(dev))
    thresh = float(torch.quantile(code_scores(lut, score_fn), 0.8))  # a prompt that keeps the top fifth of the codes
    out = render_gui(cam, pc, torch.zeros(3, device=dev))
    bg = torch.zeros(H * W, dtype=torch.bool, device=dev)
    sim = compute_similarity(out["semantics"], mlp, lut, score_fn, thresh, out_bg_mask=bg)
    # the scores of this random hyperplane lie around 0.5: lift the kept ones above the heat threshold as a prompt's are
    sim = torch.where(bg, sim, 0.7 + 0.3 * sim).contiguous()
    image = out["image"].contiguous()
    del pc
    torch.cuda.synchronize()
    return image, sim, bg


def reference_stage(image, sim, bg_mask, H, W, table, style, uint8):
    """The reference's host stage on device tensors; returns the frame (numpy, host)."""
    buffer_image = image.permute(1, 2, 0).contiguous().clamp(0, 1).contiguous().detach().cpu().numpy()
    # clip_color(cos_sim, bg_mask, H, W, thresh=0.7, res_finetuned=False, coloring=style == "heat")
    rel = torch.clamp((sim - 0.7 - 0.05) / (sim.max() - 0.7), 0, 1)
    if style == "heat":
        heat_img = table[(rel * (table.shape[0] - 1)).long()]
        heat_img[bg_mask] = 1
        colored = heat_img.reshape(H, W, 3).contiguous().clamp(0, 1).contiguous().detach().cpu().numpy()
        alpha = 1
    else:
        colored = 1
        alpha = torch.ones_like(sim)
        alpha[~bg_mask] = 0
        alpha = alpha.reshape(H, W, 1).detach().cpu().numpy()
    opa = alpha * RATIO
    final = (colored * opa + buffer_image * (1 - opa)).clip(0, 1)
    return (final * 255).astype("uint8") if uint8 else final


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
    from goi_hyperplane_amd import _lib, display
    _lib.load()
    table = display.turbo_colormap(dev)
    sizes = [tuple(int(x) for x in args.size.split("x"))] if args.size else SIZES
    rows = []
    for W, H in sizes:
        image, sim, bg = setup(W, H, dev)
        mask = bg.view(torch.uint8)
        for style in STYLES:
            for dtype in (torch.float32, torch.uint8):
                u8 = dtype == torch.uint8
                frame = torch.empty((H, W, 3), dtype=dtype, device=dev)
                comp = lambda: display.compose(image, sim, mask, style=style, overlay_ratio=RATIO, colormap=table,  # noqa: E731
                                               dtype=dtype, out=frame)
                if args.only_compose:
                    for _ in range(args.reps + 1):
                        comp()
                    torch.cuda.synchronize()
                    continue
                pinned = torch.empty((H, W, 3), dtype=dtype).pin_memory()

                def compose_and_copy():
                    comp()
                    pinned.copy_(frame, non_blocking=True)
                    return pinned

                b_ms, got = host_ms(compose_and_copy, args.reps)
                a_ms, want = host_ms(lambda: reference_stage(image, sim, bg, H, W, table, style, u8), args.reps)
                c_ms = event_ms(comp, args.reps)
                equal = bool(np.array_equal(got.numpy(), want))
                moved = bytes_moved(style, u8, H * W, int(table.shape[0]))
                rows.append({"W": W, "H": H, "style": style, "dtype": "uint8" if u8 else "float32",
                             "a_reference_stage_ms": round(a_ms, 3), "b_compose_and_pinned_copy_ms": round(b_ms, 4),
                             "c_compose_device_events_ms": round(c_ms, 4), "a_over_b": round(a_ms / b_ms, 2),
                             "frames_equal": equal, "background_share": round(float(bg.float().mean()), 4),
                             "bytes_moved": moved,
                             "bytes_over_event_time_share_of_hbm_peak": round(sum(moved.values()) / (c_ms * 1e-3)
                                                                              / HBM_PEAK_BYTES_PER_S, 4)})
                print(json.dumps(rows[-1]), flush=True)
        del image, sim, bg
    if args.only_compose:
        return None
    return {
        "what": "the viewer's frame stage: (a) the reference's host stage restated (device tensors -> .cpu().numpy() "
                "copies -> numpy blend), (b) display.compose + one device->host copy into a pinned buffer, (c) "
                "display.compose alone by device events; tools/display_time.py",
        "device": torch.cuda.get_device_name(dev), "scene": "headline (1 M Gaussians), make_orbit_cameras view 0",
        "reps": args.reps, "overlay_ratio": RATIO, "statistic": "median of reps after one warm-up, one process",
        "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
        "cache_note": "the inputs were written by the render and the decode just before and the same buffers are reused by "
                      "every repetition, so they may be cache-resident: bytes over time is not a measurement of HBM traffic",
        "rows": rows,
    }


def kernel_split(csv_path, W, H):
    """The display kernels of a rocprofv3 --stats kernel_stats.csv of --only-compose --size WxH, each with the bytes it must
    move and their share of the HBM peak at its average time."""
    with open(csv_path) as fh:
        rows = list(csv.DictReader(fh))
    out = []
    for r in rows:
        name = r["Name"]
        if "frame_" not in name:
            continue
        row = {"kernel": name[:120], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3),
               "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
        for style in STYLES:
            for u8 in (False, True):
                if f"frame_compose_k<{STYLE_CODE[style]}, {'unsigned char' if u8 else 'float'}>" in name:
                    b = bytes_moved(style, u8, H * W)["frame_compose_k"]
                    row.update(style=style, dtype="uint8" if u8 else "float32", bytes=b,
                               share_of_hbm_peak=round(b / (float(r["AverageNs"]) * 1e-9) / HBM_PEAK_BYTES_PER_S, 4))
        if "frame_stats_k" in name:
            b = bytes_moved("heat", False, H * W)["frame_stats_k"]
            row.update(bytes=b, share_of_hbm_peak=round(b / (float(r["AverageNs"]) * 1e-9) / HBM_PEAK_BYTES_PER_S, 4))
        out.append(row)
    return {"source": f"rocprofv3 --kernel-trace --stats of tools/display_time.py --only-compose --size {W}x{H}", "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", help="WxH: this frame size only")
    ap.add_argument("--only-compose", action="store_true", help="display.compose only (for the rocprofv3 kernel split)")
    ap.add_argument("--kernel-stats", help="merge a rocprofv3 kernel_stats.csv of --only-compose --size WxH into --out (no GPU)")
    args = ap.parse_args()
    if args.kernel_stats:
        if not args.size:
            ap.error("--kernel-stats needs the --size of that run")
        W, H = (int(x) for x in args.size.split("x"))
        with open(args.out) as fh:
            doc = json.load(fh)
        doc.setdefault("kernel_split", {})[args.size] = kernel_split(args.kernel_stats, W, H)
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
