"""Times the hyperplane fine-tune (gui/main.py:1673-1763) on the GPU at the reference's shape (300 codes, D = 256,
S = 16) and two frame sizes: fit_hyperplane (decode + counts + the one-launch fit) to convergence and forced to all
8000 epochs (target_iou > 1), against the reference's per-pixel LinearSVM.step loop on the same GPU, run in full.
Host clock around a device synchronisation, after one warm-up, median of 3.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` (a separate run).

    python tools/osh_time.py [--out profiles/osh_fit.json] [--sizes 512x512,1600x1056] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, _decode_idx, fit_hyperplane  # noqa: E402

dev = torch.device("cuda:0")
S, C, D = 16, 300, 256


def frame(H, W):
    torch.manual_seed(0)
    sem = torch.randn(S, H, W, device=dev)
    mlp = SemanticModel(dim_in=S, dim_out=C, num_layer=1, use_bias=True, device=dev)
    pos_code = torch.rand(C, device=dev) < 0.3
    u = torch.nn.functional.normalize(torch.randn(D, device=dev), dim=0)
    lut = torch.randn(C, D, device=dev) * 0.1 + 0.2 * (2 * pos_code.float() - 1)[:, None] * u[None]
    text = torch.nn.functional.normalize(0.3 * u + 0.7 * torch.nn.functional.normalize(torch.randn(D, device=dev), dim=0), dim=0)
    idx = _decode_idx(sem, mlp, C).long()
    return sem, mlp, lut, pos_code[idx], text, idx


def timed(fn, reps):
    fn()  # warm-up
    ts, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "osh_fit.json"))
    ap.add_argument("--sizes", default="512x512,1600x1056")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-per-pixel", action="store_true", help="skip the per-pixel loop (kernel-trace runs)")
    a = ap.parse_args()
    res = {"shape": {"n_codes": C, "D": D, "S": S}, "method": f"host clock around a synchronise, 1 warm-up, median of {a.reps}",
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for size in a.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        sem, mlp, lut, positive, text, idx = frame(H, W)

        def fused(target):
            svm = LinearSVM().to(dev)
            svm.weight_set(text.reshape(1, -1))
            return fit_hyperplane(sem, mlp, lut, positive, svm, max_epochs=8000, target_iou=target)

        def per_pixel(target):
            svm = LinearSVM().to(dev)
            svm.weight_set(text.reshape(1, -1))
            feat = lut[idx]
            normed = feat / feat.norm(dim=-1, keepdim=True)
            gt = positive.float().reshape(-1, 1)
            epoch, iou = 0, 0
            svm.eval_forward(normed, gt)
            while epoch < 8000 and iou < target:
                _, iou = svm.step(normed, gt)
                epoch += 1
            return epoch, iou

        r = {}
        for tag, target in (("converge", 0.9), ("full_8000", 1.5)):
            ms, ts, fit = timed(lambda: fused(target), a.reps)
            r[f"fused_{tag}"] = {"ms": ms, "runs_ms": ts, "epochs": fit.epochs, "iou": fit.iou, "us_per_epoch": ms * 1e3 / fit.epochs}
            print(f"{W}x{H} fused {tag}: {ms:.3f} ms, {fit.epochs} epochs, iou {fit.iou:.4f}", flush=True)
            if not a.no_per_pixel:
                ms_p, ts_p, (ep, iou) = timed(lambda: per_pixel(target), a.reps)
                r[f"per_pixel_{tag}"] = {"ms": ms_p, "runs_ms": ts_p, "epochs": ep, "iou": iou, "us_per_epoch": ms_p * 1e3 / ep}
                r[f"speedup_{tag}"] = ms_p / ms
                print(f"{W}x{H} per-pixel {tag}: {ms_p:.1f} ms, {ep} epochs, iou {iou:.4f} -> x{ms_p / ms:.1f}", flush=True)
        res["sizes"][f"{W}x{H}"] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
