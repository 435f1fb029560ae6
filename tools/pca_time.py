"""Times the PCA picture of the semantic features (goi_hyperplane_amd/pca.py, csrc/pca.hip) on feature maps of
1600 x 1056 x 16 and 800 x 800 x 10, resident on the device, and writes profiles/pca.json:

    accumulate      the moments of one map (pivot + the streaming kernel): the bytes of the map over this time is the
                    share of the streaming bandwidth
    solve           slot reduction + the fp64 Jacobi of one wave
    fit             accumulate + solve
    apply_*         the projection, raw / sigma (one launch) and minmax (two)
    fit_apply       what a frame with its own basis costs: fit + apply (sigma)
    torch           the same stage restated in torch on the same device: torch.cov + torch.linalg.eigh + matmul
    reference       the reference's stage restated: the map's .cpu().numpy(), sklearn PCA(3).fit_transform on its HW x S rows
                    (host clock around it; "absent" without scikit-learn)

The device figures are medians over --rounds of windows of --iters calls between two device events, the variants
ALTERNATING inside a round, after one warm-up round.  Every call of a window takes the next of --maps different maps
(together larger than the 256 MB last-level cache), so a map is not cache-resident when its turn comes.

    python tools/pca_time.py [--out profiles/pca.json] [--rounds 7] [--iters 8]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SIZES = ((1600, 1056, 16), (800, 800, 10))
STREAM_BYTES_PER_S = 6.29e12  # a float4 copy on this device (8.0e12 is the data sheet's HBM peak)
HBM_PEAK_BYTES_PER_S = 8.0e12


def feature_maps(S, H, W, count, dev):
    """`count` different maps with a few dominant directions about a non-zero mean, as a trained feature field has."""
    g = torch.Generator(device=dev).manual_seed(S * H + W)
    maps = []
    for _ in range(count):
        z = torch.randn(4, H * W, device=dev, generator=g) * torch.tensor([4.0, 2.0, 1.0, 0.5], device=dev)[:, None]
        mix = torch.randn(S, 4, device=dev, generator=g) / 2
        x = mix @ z + 0.05 * torch.randn(S, H * W, device=dev, generator=g) + torch.randn(S, 1, device=dev, generator=g)
        maps.append(x.reshape(S, H, W).contiguous())
    return maps


def torch_stage(x):
    S = x.shape[0]
    X = x.reshape(S, -1)
    w, v = torch.linalg.eigh(torch.cov(X))
    return v[:, -3:].flip(1).T @ (X - X.mean(dim=1, keepdim=True))


def reference_stage(x):
    from sklearn.decomposition import PCA
    rows = x.permute(1, 2, 0).reshape(-1, x.shape[0]).cpu().numpy()
    return PCA(n_components=3).fit_transform(rows)


def window_ms(fn, maps, iters, at):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(maps[(at + i) % len(maps)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def measure(args, dev):
    from goi_hyperplane_amd import _lib, pca
    _lib.load()
    rows = []
    for W, H, S in SIZES:
        maps = feature_maps(S, H, W, args.maps, dev)
        fit = pca.Fit(S, dev)
        basis = pca.fit(maps[0])
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        variants = {
            "accumulate": lambda x: fit.reset().add(x),
            "solve": lambda x: fit.solve(),
            "fit": lambda x: fit.reset().add(x).solve(),
            "apply_raw": lambda x: pca.transform(x, basis, normalize="raw", out=out),
            "apply_sigma": lambda x: pca.transform(x, basis, normalize="sigma", out=out),
            "apply_minmax": lambda x: pca.transform(x, basis, normalize="minmax", out=out),
            "fit_apply": lambda x: pca.transform(x, fit.reset().add(x).solve(), normalize="sigma", out=out),
        }
        note = {}
        try:
            torch_stage(maps[0])
            torch.cuda.synchronize()
            variants["torch"] = torch_stage
        except Exception as ex:  # noqa: BLE001 -- a build of torch without a device eigh: named, not hidden
            note["torch"] = f"not measured: {type(ex).__name__}: {str(ex)[:200]}"
        times = {k: [] for k in variants}
        at = 0
        for r in range(args.rounds + 1):
            for name, fn in variants.items():
                ms = window_ms(fn, maps, args.iters, at)
                at += args.iters
                if r:
                    times[name].append(ms)
        row = {"W": W, "H": H, "S": S, "map_bytes": S * H * W * 4}
        for name, ts in times.items():
            row[name + "_ms"] = round(statistics.median(ts), 4)
            row[name + "_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
        row.update(note)
        bps = row["map_bytes"] / (row["accumulate_ms"] * 1e-3)
        row["accumulate_bytes_per_s"] = round(bps, -9)
        row["accumulate_share_of_streaming_bandwidth"] = round(bps / STREAM_BYTES_PER_S, 4)
        row["accumulate_share_of_hbm_peak"] = round(bps / HBM_PEAK_BYTES_PER_S, 4)
        apply_bytes = row["map_bytes"] + 3 * H * W * 4
        row["apply_sigma_share_of_streaming_bandwidth"] = round(apply_bytes / (row["apply_sigma_ms"] * 1e-3) / STREAM_BYTES_PER_S, 4)
        try:
            import sklearn
            ts = []
            for r in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                reference_stage(maps[r % len(maps)])
                if r:
                    ts.append((time.perf_counter() - t0) * 1e3)
            row["reference_ms"] = round(statistics.median(ts), 2)
            row["reference"] = f"scikit-learn {sklearn.__version__}: .cpu().numpy() + PCA(3).fit_transform, host clock, median of 2 after one warm-up"
        except ImportError:
            row["reference"] = "absent: scikit-learn is not installed on this machine"
        rows.append(row)
        print(json.dumps(row), flush=True)
        del maps
    return {
        "what": "the PCA picture of the semantic features: csrc/pca.hip against a torch restatement on the same device and "
                "the reference's host stage; tools/pca_time.py",
        "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "iters_per_window": args.iters, "maps": args.maps,
        "statistic": "median (and min, max) over the rounds of a window's time per call by device events, variants alternating "
                     "inside a round, one warm-up round; the maps rotate so that none is cache-resident",
        "streaming_bytes_per_s": STREAM_BYTES_PER_S, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
        "rows": rows,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--maps", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pca_time.py needs a ROCm device: a time taken anywhere else says nothing")
    doc = measure(args, torch.device("cuda:0"))
    print(json.dumps(doc, indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
