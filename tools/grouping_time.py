"""Times the fused mask-contrast loss (goi_hyperplane_amd.grouping, csrc/grouping.hip) and writes
profiles/grouping.json.

    Shapes 1600x1056x16 and 800x528x16; label maps with margin 1:
      uniform        one mask over the whole map: every sum lands on the same S + 1 words -- the worst case for the atomics;
      voronoi_64     64 Voronoi cells;   voronoi_300   300 cells (a mask generator's typical output);
      checker_2      a 1-pixel checkerboard of two labels: every lane hands its run over at every pixel;
      random_64      a random label below 64 per pixel: every lane of a wave another label.
    ALTERNATING in one process, per shape and map: the loss with its gradient, the loss alone, both again with max_abs given (no
    pass for the maximum), and THE OTHER ROUTE -- the torch restatement on the same device: permute, index_add_ (float atomics),
    gather, the K x K pair block, autograd's mirror of it all.
    Floor: the compulsory traffic -- feat twice (three times with the pass for the maximum), labels twice, grad once -- over the
    streaming figure README.md measures the device by.

A window is two device events around one call and ends in a synchronise; per form the median, quartiles, extremes and the
medians of the two halves of the windows.  The per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of
--only-loss (one shape and map per run), merged with --kernel-stats.  Needs a GPU.

    python tools/grouping_time.py [--out profiles/grouping.json] [--reps 10]
    python tools/grouping_time.py --only-loss --size 1600x1056 --layout uniform          (the driver of a rocprofv3 run)
    python tools/grouping_time.py --kernel-stats kernel_stats.csv --size 1600x1056 --layout uniform
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tools.contrib_time import alternate  # noqa: E402
from tools.knn_time import STREAM_TBS  # noqa: E402

S = 16
SIZES = ((1600, 1056), (800, 528))
LAYOUTS = ("uniform", "voronoi_64", "voronoi_300", "checker_2", "random_64")


def label_map(layout, W, H, dev):
    """-> (labels int32 [H,W], K)"""
    g = torch.Generator(device=dev).manual_seed(3)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    if layout == "uniform":
        return torch.zeros((H, W), dtype=torch.int32, device=dev), 1
    if layout == "checker_2":
        return ((yy + xx) & 1).to(torch.int32), 2
    if layout == "random_64":
        return torch.randint(0, 64, (H, W), device=dev, generator=g, dtype=torch.int32), 64
    K = int(layout.split("_")[1])
    sites = torch.rand((K, 2), device=dev, generator=g) * torch.tensor([H, W], device=dev)
    best = torch.full((H, W), float("inf"), device=dev)
    lab = torch.zeros((H, W), dtype=torch.int32, device=dev)
    for k in range(K):  # (K passes over the map rather than an [H,W,K] block)
        d = (yy - sites[k, 0]) ** 2 + (xx - sites[k, 1]) ** 2
        lab = torch.where(d < best, torch.full_like(lab, k), lab)
        best = torch.minimum(best, d)
    return lab, K


def feature_map(labels, K, dev):
    """a centre per mask about one margin from the others, plus noise: some pairs pull, some do not"""
    g = torch.Generator(device=dev).manual_seed(4)
    centres = torch.randn((K, S), device=dev, generator=g) * (0.8 / S ** 0.5)
    f = centres[labels.long()] + torch.randn((*labels.shape, S), device=dev, generator=g) * (0.5 / S ** 0.5)
    return f.permute(2, 0, 1).contiguous()


def torch_loss(feat, labels, K, margin=1.0):
    """the restatement a user would write: permute, index_add_, gather, pair block (balance = "pixel", both weights 1)"""
    Sx = feat.shape[0]
    f = feat.permute(1, 2, 0).reshape(-1, Sx)
    lab = labels.reshape(-1).long()
    ok = (lab >= 0) & (lab < K)
    f, lab = f[ok], lab[ok]
    n = torch.zeros(K, device=f.device).index_add_(0, lab, torch.ones_like(lab, dtype=torch.float32))
    mu = torch.zeros((K, Sx), device=f.device).index_add_(0, lab, f) / n.clamp_min(1)[:, None]
    intra = ((f - mu[lab]) ** 2).sum() / n.sum().clamp_min(1)
    live = n > 0
    M = live.sum()
    d2 = ((mu[:, None, :] - mu[None, :, :]) ** 2).sum(-1)
    pairs = live[:, None] & live[None, :] & ~torch.eye(K, dtype=torch.bool, device=f.device)
    d = torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2)))
    pair = torch.where(d2 > 0, torch.clamp(margin - d, min=0) ** 2, torch.full_like(d2, margin * margin))
    inter = (pair * pairs).sum() / (M * (M - 1)).clamp_min(1)
    return intra + inter


def floor(W, H, with_max, with_grad):
    feat = S * H * W * 4
    b = feat * (3 if with_max else 2) + 2 * H * W * 4 + (feat if with_grad else 0)
    return b, b / (STREAM_TBS * 1e12) * 1e3


def row(layout, W, H, dev, reps):
    from goi_hyperplane_amd import grouping
    labels, K = label_map(layout, W, H, dev)
    feat = feature_map(labels, K, dev)
    top = float(feat.abs().max().cpu())
    leaf = feat.clone().requires_grad_(True)

    def fused(f, **kw):
        return lambda: grouping.loss_terms(f, labels, K, **kw)

    def other():
        leaf.grad = None
        torch_loss(leaf, labels, K).backward()

    nothing = lambda: None  # noqa: E731
    forms = {"loss_and_grad": (nothing, fused(leaf)), "loss_alone": (nothing, fused(feat)),
             "loss_and_grad_max_abs": (nothing, fused(leaf, max_abs=top)), "loss_alone_max_abs": (nothing, fused(feat, max_abs=top)),
             "torch_loss_and_grad": (nothing, other), "torch_loss_alone": (nothing, lambda: torch_loss(feat, labels, K))}
    res = alternate(forms, reps)
    med = {n: r["median_ms"] for n, r in res.items()}
    # outside the windows: the routes agree to float32 noise, and a second call repeats
    a, b = grouping.loss_terms(leaf, labels, K), grouping.loss_terms(leaf, labels, K)
    other()
    first = leaf.grad.clone()
    other()
    floors = {}
    for name, with_max, with_grad in (("loss_and_grad", True, True), ("loss_alone", True, False), ("loss_and_grad_max_abs", False, True),
                                      ("loss_alone_max_abs", False, False)):
        nbytes, ms = floor(W, H, with_max, with_grad)
        floors[name] = {"compulsory_bytes": nbytes, "floor_ms": round(ms, 4), "time_over_floor": round(med[name] / ms, 2)}
    return {"layout": layout, "W": W, "H": H, "S": S, "K": K, "windows": res,
            "torch_over_fused_loss_and_grad": round(med["torch_loss_and_grad"] / med["loss_and_grad"], 2),
            "torch_over_fused_loss_alone": round(med["torch_loss_alone"] / med["loss_alone"], 2),
            "floor": floors,
            "loss": float(a[0].detach().cpu()), "torch_loss": float(torch_loss(feat, labels, K).cpu()),
            "largest_gradient_difference_from_torch": float((a[3] - first).abs().max().cpu()),
            "largest_gradient": float(a[3].abs().max().cpu()),
            "same_bits_on_a_second_call": bool(torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))
                                               and torch.equal(a[0].detach().view(torch.int32), b[0].detach().view(torch.int32))),
            "torch_same_bits_on_a_second_call": bool(torch.equal(first.view(torch.int32), leaf.grad.view(torch.int32)))}


def kernel_split(csv_path, W, H, layout):
    """The grp_* kernels of a rocprofv3 --stats kernel_stats.csv of --only-loss, each with the bytes it must move and what share of
    the streaming figure that is at its average time."""
    feat, lab = S * H * W * 4, H * W * 4
    must = {"grp_max_k": feat, "grp_sums_k": feat + lab, "grp_grad_k": 2 * feat + lab}
    with open(csv_path) as fh:
        rows = list(csv.DictReader(fh))
    out = []
    for r in rows:
        if "grp_" not in r["Name"]:
            continue
        k = {"kernel": r["Name"][:100], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 3),
             "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
        for name, b in must.items():
            if name in r["Name"]:
                k.update(bytes=b, share_of_streaming=round(b / (float(r["AverageNs"]) * 1e-9) / (STREAM_TBS * 1e12), 4))
        out.append(k)
    return {"source": f"rocprofv3 --kernel-trace --stats of tools/grouping_time.py --only-loss --size {W}x{H} --layout {layout}",
            "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouping.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", help="WxH: this shape only")
    ap.add_argument("--layout", choices=LAYOUTS, help="this label map only")
    ap.add_argument("--only-loss", action="store_true", help="grouping.loss with its gradient only (for the rocprofv3 kernel split)")
    ap.add_argument("--kernel-stats", help="merge a rocprofv3 kernel_stats.csv of --only-loss --size WxH --layout L into --out (no GPU)")
    args = ap.parse_args()
    sizes = [tuple(int(x) for x in args.size.split("x"))] if args.size else SIZES
    layouts = [args.layout] if args.layout else LAYOUTS
    if args.kernel_stats:
        if not (args.size and args.layout):
            ap.error("--kernel-stats needs the --size and --layout of that run")
        with open(args.out) as fh:
            doc = json.load(fh)
        doc.setdefault("kernel_split", {})[f"{args.size}_{args.layout}"] = kernel_split(args.kernel_stats, *sizes[0], args.layout)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
        return
    assert torch.cuda.is_available(), "tools/grouping_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _lib, grouping
    _lib.load()
    if args.only_loss:
        (W, H), layout = sizes[0], layouts[0]
        labels, K = label_map(layout, W, H, dev)
        feat = feature_map(labels, K, dev).requires_grad_(True)
        for _ in range(3 + args.reps):
            grouping.loss_terms(feat, labels, K)
        torch.cuda.synchronize()
        return
    doc = {"what": "the fused mask-contrast loss (goi_hyperplane_amd.grouping) next to its torch restatement (permute, index_add_, gather, "
                   "pair block, autograd) on the same device; tools/grouping_time.py",
           "device": torch.cuda.get_device_name(dev),
           "statistic": "two device events around one call, the window ending in a synchronise; forms alternate in one process after "
                        "warm-up; median, quartiles, extremes, medians of the two halves",
           "streaming_TB_per_s": STREAM_TBS, "rows": []}
    for W, H in sizes:
        for layout in layouts:
            r = row(layout, W, H, dev, args.reps)
            print(json.dumps({k: v for k, v in r.items() if k != "windows"} | {"median_ms": {n: w["median_ms"] for n, w in r["windows"].items()}}),
                  flush=True)
            doc["rows"].append(r)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
