"""Times the code-book initialisation of train.py:78-86 and writes profiles/codebook_init.json.

Workload: --views APE maps of [256, 528, 800] fp32 (800 x 528 pixels), each piecewise constant over ~150 segments
(random 256-d embeddings on a random 16 x 16-pixel block labelling) plus a zero region (unlabelled pixels); the maps
come from one seed, so both sides see the same data.

    (a) reference: the stage restated -- per view m.permute(1, 2, 0).reshape(-1, 256).unique(dim=0) on the CPU,
        .cuda(), io.kmeans(., 80) on the GPU; then io.kmeans(tot, 300).  Maps on the host (where the reference's
        dataset reader leaves them).  Timed once (it takes about a minute).
    (b) semantic.init_codebook with the maps on the host: staged through pinned buffers (CODEBOOK_STAGING "pinned") and
        with plain pageable copies ("pageable").
    (c) semantic.init_codebook with the maps already on the device; and unique_rows alone on them.
    (d) adversarial dedup: unique_rows of one view whose 422 400 rows are all distinct (the radix-sort path).
Host clock around a synchronisation; median of --reps after one warm-up, same process, same seed for both sides.  The
LUTs of (a) and (b) are compared (same RNG draws; the means differ in summation order only).  The per-kernel split comes
from a separate `rocprofv3 --kernel-trace --stats` run of --only-gpu.

    python tools/codebook_init_time.py [--out profiles/codebook_init.json] [--views 25] [--reps 3]
    python tools/codebook_init_time.py --only-gpu --views 4 --reps 1        (the driver of the rocprofv3 run)
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

D, H, W = 256, 528, 800


def make_maps(views, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    maps = []
    for _ in range(views):
        emb = torch.randn(150, D, generator=g, device=dev)
        emb[0] = 0  # unlabelled pixels
        lab = torch.randint(1, 150, (H // 16, W // 16), generator=g, device=dev)
        lab[: H // 64, : W // 4] = 0  # a zero region
        lab = lab.repeat_interleave(16, 0).repeat_interleave(16, 1)
        maps.append(emb[lab].permute(2, 0, 1).contiguous().cpu())
    return maps


def clock(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t, out


def timed(fn, dev, reps):
    clock(fn, dev)  # warm-up
    ts = []
    out = None
    for _ in range(reps):
        t, out = clock(fn, dev)
        ts.append(t)
    return statistics.median(ts), ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codebook_init.json"))
    ap.add_argument("--views", type=int, default=25)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only-gpu", action="store_true")
    a = ap.parse_args()
    from goi_hyperplane_amd import io as gio
    from goi_hyperplane_amd import semantic
    dev = torch.device("cuda", 0)
    maps = make_maps(a.views, a.seed, dev)
    res = {"workload": {"views": a.views, "D": D, "H": H, "W": W, "segments": 150, "zero_region": True, "seed": a.seed,
                        "map_MB": D * H * W * 4 / 1e6},
           "reps": a.reps, "device": torch.cuda.get_device_name(dev)}

    def ours():
        torch.manual_seed(a.seed)
        return semantic.init_codebook(maps)

    res["uniques_per_view"] = [int(u.shape[0]) for u in semantic.unique_rows(maps)]
    for mode in ("pinned", "pageable"):
        semantic.CODEBOOK_STAGING = mode
        med, ts, lut = timed(ours, dev, a.reps)
        res[f"init_codebook_host_{mode}_s"] = med
        res[f"init_codebook_host_{mode}_runs_s"] = ts
    semantic.CODEBOOK_STAGING = "pinned"
    dmaps = [m.to(dev) for m in maps]

    def ours_dev():
        torch.manual_seed(a.seed)
        return semantic.init_codebook(dmaps)

    med, ts, lut_dev = timed(ours_dev, dev, a.reps)
    res["init_codebook_device_s"], res["init_codebook_device_runs_s"] = med, ts
    med, ts, _ = timed(lambda: semantic.unique_rows(dmaps), dev, a.reps)
    res["unique_rows_device_s"], res["unique_rows_device_per_view_ms"] = med, med / a.views * 1e3
    uniq = semantic.unique_rows(dmaps)

    def km():
        torch.manual_seed(a.seed)
        tot = torch.cat(semantic.spherical_kmeans_batched([u.clone() for u in uniq], 80), 0)
        return semantic.spherical_kmeans(tot, 300)

    res["kmeans_two_levels_device_s"] = timed(km, dev, a.reps)[0]
    res["copy_host_to_device_pageable_s"] = timed(lambda: [m.to(dev) for m in maps], dev, a.reps)[0]
    del dmaps
    adv = torch.randn(D, H, W, device=dev)
    med, ts, u = timed(lambda: semantic.unique_rows(adv), dev, a.reps)
    res["adversarial_all_distinct"] = {"rows": int(u[0].shape[0]), "unique_rows_device_s": med, "runs_s": ts}
    del adv, u
    torch.cuda.synchronize(dev)
    if not a.only_gpu:
        def reference():
            torch.manual_seed(a.seed)
            tot = torch.cat([gio.kmeans(m.permute(1, 2, 0).reshape(-1, D).unique(dim=0).cuda(), 80) for m in maps], 0)
            return gio.kmeans(tot, 300).float()

        t0 = time.perf_counter()
        u0 = maps[0].permute(1, 2, 0).reshape(-1, D).unique(dim=0)
        res["reference_cpu_unique_one_view_s"] = time.perf_counter() - t0
        del u0
        t, lut_ref = clock(reference, dev)
        res["reference_stage_s"] = t
        res["torch_threads"] = torch.get_num_threads()
        res["speedup_host_maps"] = t / min(res["init_codebook_host_pinned_s"], res["init_codebook_host_pageable_s"])
        res["speedup_device_maps"] = t / res["init_codebook_device_s"]
        diff = (lut_ref - lut).abs()
        res["lut_vs_reference"] = {"max_abs_diff": float(diff.nan_to_num(0).max()),
                                   "nan_rows_equal": bool(torch.equal(lut_ref.isnan(), lut.isnan())),
                                   "allclose_2e-6": bool(torch.allclose(lut_ref, lut, rtol=0, atol=2e-6, equal_nan=True))}
    res["lut_host_equals_lut_device"] = bool(torch.equal(lut.nan_to_num(7), lut_dev.nan_to_num(7)))
    print(json.dumps(res, indent=1))
    if not a.only_gpu:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
