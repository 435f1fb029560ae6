"""Times goi_hyperplane_amd.densify and writes profiles/densify.json.

At 1 M and 3 M Gaussians (SH degree 3, S = 16, a stepped 7-group FusedAdam, about 5 % clone / 5 % split / 3 % prune):
densify_and_prune, prune_points and add_densification_stats on the HIP path against the restatement of the reference's
methods (tests/densify_reference.py) on the same GPU.  Device events around each call after warm-up, median over --reps
calls; every call starts from a fresh copy of the model (the copy is outside the timed window).  The apply kernel's byte
floor is 900 (P + P') B -- one read of the old rows and one write of the new ones, parameters and both moments -- plus the
plan's 24 B per Gaussian.  Its achieved share of 6.3 TB/s needs kernel times, which come from a separate
`rocprofv3 --kernel-trace` run of --only-hip; --merge-trace adds their medians per size to the JSON (no GPU needed).

    python tools/densify_time.py --out densify.json [--reps 7]                         (events, both arms)
    rocprofv3 --kernel-trace --output-format csv -d prof -o densify -- \
        python tools/densify_time.py --only-hip --reps 3                              (kernel times)
    python tools/densify_time.py --merge-trace prof/densify_kernel_trace.csv --json densify.json \
        --out profiles/densify.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM = 6.3e12  # bytes/s


def model(P, dev):
    from tests import densify_reference as ref
    # grads spread so that ~5 % clone and ~5 % split; opacities so that ~3 % are pruned
    m = ref.make_model(P, dev, seed=1, optimizer="fused", max_grad=2e-4, min_opacity=0.1, denom_zero=0.0)
    with torch.no_grad():
        g = torch.Generator(device=dev).manual_seed(2)
        m.xyz_gradient_accum.copy_(m.denom * 2e-4 * (0.1 + 0.9 * torch.rand(P, 1, device=dev, generator=g)))
        hot = torch.rand(P, 1, device=dev, generator=g) < 0.1
        m.xyz_gradient_accum.copy_(torch.where(hot, m.denom * 3e-4, m.xyz_gradient_accum))
        m._opacity.copy_(torch.where(torch.rand(P, 1, device=dev, generator=g) < 0.03, torch.full_like(m._opacity, -4.0),
                                     torch.full_like(m._opacity, 1.0)))
    return m


def clone_model(m):
    from goi_hyperplane_amd.optim import FusedAdam
    from tests import densify_reference as ref
    c = ref.Model()
    c.percent_dense = m.percent_dense
    for _, attr in ref.PARAMS:
        setattr(c, attr, torch.nn.Parameter(getattr(m, attr).detach().clone()))
    for name in ref.STATS:
        setattr(c, name, getattr(m, name).clone())
    groups = [{"params": [getattr(c, ref.ATTR[g["name"]])], "lr": g["lr"], "name": g["name"]} for g in m.optimizer.param_groups]
    c.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
    for g, gc in zip(m.optimizer.param_groups, c.optimizer.param_groups):
        st = m.optimizer.state[g["params"][0]]
        c.optimizer.state[gc["params"][0]] = {"step": st["step"].clone(), "exp_avg": st["exp_avg"].clone(),
                                              "exp_avg_sq": st["exp_avg_sq"].clone()}
    return c


def timed(fn, reps, dev, setup):
    out = []
    for _ in range(reps):
        arg = setup()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(arg)
        b.record()
        torch.cuda.synchronize(dev)
        out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(out), "min_us": min(out)}


def case(P, args, dev):
    from goi_hyperplane_amd import densify
    from tests import densify_reference as ref
    base = model(P, dev)
    mask = torch.rand(P, device=dev, generator=torch.Generator(device=dev).manual_seed(4)) < 0.05
    vp = torch.zeros(P, 3, device=dev, requires_grad=True)
    vp.grad = torch.randn(P, 3, device=dev) * 1e-3
    filt = torch.rand(P, device=dev) < 0.6
    arms = {"hip": (densify.densify_and_prune, densify.prune_points, densify.add_densification_stats)}
    if not args.only_hip:
        arms["restated"] = (ref.densify_and_prune, ref.prune_points, ref.add_densification_stats)
    res = {"P": P}
    for name, (dp, pp, st) in arms.items():
        warm = clone_model(base)
        dp(warm, 2e-4, 0.1, 4.0, None)
        r = {"densify_and_prune": timed(lambda m: dp(m, 2e-4, 0.1, 4.0, None), args.reps, dev, lambda: clone_model(base)),
             "prune_points": timed(lambda m: pp(m, mask), args.reps, dev, lambda: clone_model(base)),
             "add_densification_stats": timed(lambda m: st(m, vp, filt), args.reps, dev, lambda: clone_model(base))}
        res[name] = r
    after = clone_model(base)
    densify.densify_and_prune(after, 2e-4, 0.1, 4.0, None)
    Pn = after._xyz.shape[0]
    res["P_new"] = Pn
    row = sum(getattr(base, a).numel() // P for _, a in ref.PARAMS) * 4 * 3
    res["row_bytes_params_and_moments"] = row
    res["apply_floor_bytes"] = row * (P + Pn)
    res["apply_floor_us"] = res["apply_floor_bytes"] / HBM * 1e6
    res["plan_floor_bytes"] = 24 * P
    res["stats_floor_bytes"] = (12 + 1 + 16) * P
    if "restated" in res:
        res["speedup_densify_and_prune"] = (res["restated"]["densify_and_prune"]["median_us"] /
                                           res["hip"]["densify_and_prune"]["median_us"])
    return res


KERNELS = ("densify_plan_k", "densify_stats_k", "prune_plan_k", "densify_apply_k")


def merge_trace(res, trace_csv):
    """adds, per size, the median kernel times of a rocprofv3 --kernel-trace CSV of an --only-hip run of the same sizes.
    Plan / statistics kernels are told apart by their grid (P rounded up to 256); the apply launches of a size by their
    grid too: the larger grid is densify_and_prune's (it also writes the new rows), the smaller prune_points'."""
    import csv
    by = {k: [] for k in KERNELS}
    with open(trace_csv) as fh:
        for r in csv.DictReader(fh):
            for k in by:
                if "::" + k + "(" in r["Kernel_Name"]:
                    grid = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y") or 1)
                    by[k].append((grid, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    for c in res["cases"]:
        P = c["P"]
        pad = (P + 255) // 256 * 256
        kk = {k + "_us": statistics.median([d for g, d in by[k] if g == pad]) for k in KERNELS[:3]}
        row_floats = c["row_bytes_params_and_moments"] // 12
        expect = 3 * row_floats * P / 4  # work-items: one per 4 source floats of the parameters and both moments
        mine = sorted({g for g, _ in by["densify_apply_k"] if abs(g - expect) < 0.25 * expect})
        kk["densify_apply_k_us (densify_and_prune)"] = statistics.median([d for g, d in by["densify_apply_k"] if g == mine[-1]])
        kk["densify_apply_k_us (prune_points)"] = statistics.median([d for g, d in by["densify_apply_k"] if g == mine[0]])
        kk["apply_share_of_6.3TB/s"] = round(c["apply_floor_us"] / kk["densify_apply_k_us (densify_and_prune)"], 3)
        c["kernels_rocprofv3"] = kk
    res["kernel_times"] = "kernels_rocprofv3: medians of a separate rocprofv3 --kernel-trace run of --only-hip (--merge-trace)"
    return res


def write(res, out):
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge-trace", default=None, help="rocprofv3 kernel_trace.csv to merge into --json")
    ap.add_argument("--json", default=None, help="an earlier output of this tool (with --merge-trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1000000,3000000")
    ap.add_argument("--only-hip", action="store_true")
    args = ap.parse_args()
    if args.merge_trace:
        with open(args.json) as fh:
            write(merge_trace(json.load(fh), args.merge_trace), args.out)
        return
    if not torch.cuda.is_available():
        raise SystemExit("densify_time.py measures the GPU and found none")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "cases": [case(int(P), args, dev) for P in args.sizes.split(",")]}
    write(res, args.out)


if __name__ == "__main__":
    main()
