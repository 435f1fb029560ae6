"""Times goi_hyperplane_amd.mcmc and writes profiles/mcmc.json.

At 1 M Gaussians (SH degree 3, S = 16, a stepped 7-group FusedAdam) with 1 %, 5 % and 50 % of the rows dead:

  relocate   against the same step restated in torch on the same device (sigmoid, nonzero, multinomial, bincount, the binomial
             sum as a table product, index assignment into the 7 parameters, zeroing of the sources' 14 moment rows), and --
             for scale -- against densify.densify_and_prune on the scene tools/densify_time.py times;
  add_noise  against build_rotation + bmm in torch (fp32, as a trainer would write it);
  the worst case of relocate: every draw on one source (one hot counter, N clamps at 51).

Device events around each call after warm-up; the arms ALTERNATE (one window of each per round), medians and quartiles over
--reps rounds.  Before every window the opacities are put back (outside the window), so every call sees the same dead set.
The compulsory bytes of an entry are what its definition has to move (see floor_*), the floor is those bytes at 6.29 TB/s, the
share is floor / median of the whole call -- launches, the sigmoid and the draws included: a call-level figure, not a kernel's
share of peak (kernel times would need a rocprofv3 --kernel-trace run of their own: not measured here).

    python tools/mcmc_time.py --out profiles/mcmc.json [--reps 9] [--P 1000000]
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

HBM = 6.29e12  # bytes/s, the streaming figure
ROW_FLOATS = 3 + 3 + 45 + 16 + 1 + 3 + 4


def model(P, dev, dead_share, seed=1):
    from tests import densify_reference as ref
    m = ref.make_model(P, dev, seed=seed, optimizer="fused", steps=1)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    with torch.no_grad():
        dead = torch.rand(P, 1, device=dev, generator=g) < dead_share
        m._opacity.copy_(torch.where(dead, torch.full_like(m._opacity, -8.0), m._opacity.clamp(min=-3.0)))
    return m


def table(dev):
    """A[N-1, k] = sum_{m=1..N} C(m-1, k) (-1)^k / sqrt(k+1): D = sum_k A[N-1, k] o'^(k+1)"""
    a = torch.zeros(51, 51, dtype=torch.float64)
    for m in range(1, 52):
        for k in range(m):
            a[m - 1, k] = math.comb(m - 1, k) * (-1) ** k / math.sqrt(k + 1)
    return a.cumsum(0).to(dev)


@torch.no_grad()
def torch_relocate(m, min_opacity, gen, tab):
    """the same step in torch, float64 for the sum (fp32 loses it: DESIGN 4.32); synchronises at nonzero, as any torch trainer does"""
    from tests import densify_reference as ref
    op = torch.sigmoid(m._opacity).flatten()
    dead = op <= min_opacity
    dead_idx = dead.nonzero(as_tuple=True)[0]
    alive_idx = (~dead).nonzero(as_tuple=True)[0]
    n = dead_idx.numel()
    if n == 0 or alive_idx.numel() == 0:
        return 0
    src = alive_idx[torch.multinomial(op[alive_idx], n, replacement=True, generator=gen)]
    N = (torch.bincount(src, minlength=op.numel())[src] + 1).clamp(max=51)
    o = op[src].double().clamp(max=1 - 2.0 ** -24)
    o_new = 1 - (1 - o) ** (1.0 / N.double())
    pw = o_new[:, None] ** torch.arange(1, 52, device=op.device, dtype=torch.float64)[None]
    D = (tab[N - 1] * pw).sum(1)
    new_op = torch.logit(o_new.clamp(min_opacity, 1 - 2.0 ** -24)).float()[:, None]
    new_scale = (m._scaling[src].double() + torch.log(o / D)[:, None]).float()
    for name, attr in ref.PARAMS:
        p = getattr(m, attr)
        p[dead_idx] = p[src]
        st = m.optimizer.state[p]
        st["exp_avg"][src] = 0
        st["exp_avg_sq"][src] = 0
    m._opacity[src] = new_op
    m._opacity[dead_idx] = new_op
    m._scaling[src] = new_scale
    m._scaling[dead_idx] = new_scale
    return n


@torch.no_grad()
def torch_noise(m, z, step, k=100.0, x0=0.995):
    from tests import densify_reference as ref
    R = ref.rotation_matrices(m._rotation)
    M = R * torch.exp(m._scaling)[:, None, :]
    cov = torch.bmm(M, M.transpose(1, 2))
    g = 1 / (1 + torch.exp(-k * ((1 - torch.sigmoid(m._opacity)) - x0)))
    m._xyz.add_(torch.bmm(cov, (z * g * step)[:, :, None]).squeeze(-1))


def quartiles(x):
    q = statistics.quantiles(x, n=4) if len(x) > 1 else [x[0]] * 3
    return {"median_us": statistics.median(x), "q1_us": q[0], "q3_us": q[2], "min_us": min(x)}


def alternate(arms, reps, dev, reset):
    """arms: {name: fn}; one window of each per round, in turn"""
    out = {k: [] for k in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            reset()
            torch.cuda.synchronize(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(dev)
            out[name].append(a.elapsed_time(b) * 1e3)
    return {k: quartiles(v) for k, v in out.items()}


def floor_relocate(P, moves, sources):
    """two reads of opacity (8 P), r = 0 (4 P), C (8 P), the dead ids (4 n_dead <= 4 P, counted as moves); per move its draw (8), one
    line of C (8), the counter (4), the source word written and read twice (12), the staged values written and read (32) and the 75
    floats of a row read and written (600); per source its new opacity and log-scale (16) and its 150 moment floats zeroed (600)"""
    return 20 * P + moves * (4 + 8 + 8 + 4 + 12 + 32 + 2 * 4 * ROW_FLOATS) + sources * (16 + 2 * 4 * ROW_FLOATS)


def case_relocate(P, share, args, dev):
    from goi_hyperplane_amd import mcmc
    m = model(P, dev, share)
    saved = m._opacity.detach().clone()
    tab = table(dev)
    gen = torch.Generator(device=dev).manual_seed(3)

    def reset():
        with torch.no_grad():
            m._opacity.copy_(saved)

    arms = {"hip": lambda: mcmc.relocate(m, generator=gen), "torch_restated": lambda: torch_relocate(m, 0.005, gen, tab)}
    for fn in arms.values():  # warm-up of both arms
        reset()
        fn()
    res = alternate(arms, args.reps, dev, reset)
    reset()
    counts = mcmc.relocate(m, generator=gen).cpu().tolist()
    res.update({"dead_share": share, "counts_moves_dead_alive_sources": counts})
    res["floor_bytes"] = floor_relocate(P, counts[0], counts[3])
    res["floor_us"] = res["floor_bytes"] / HBM * 1e6
    res["share_of_floor_call_level"] = round(res["floor_us"] / res["hip"]["median_us"], 4)
    res["speedup_over_torch"] = round(res["torch_restated"]["median_us"] / res["hip"]["median_us"], 2)
    # the worst case: every draw on one source
    draws = torch.zeros(P, dtype=torch.int64, device=dev)
    worst = alternate({"hip_all_draws_on_one_source": lambda: mcmc.relocate(m, draws=draws)}, args.reps, dev, reset)
    res.update(worst)
    return res


def case_noise(P, args, dev):
    from goi_hyperplane_amd import mcmc
    m = model(P, dev, 0.05)
    saved = m._xyz.detach().clone()
    z = torch.randn(P, 3, device=dev)
    step = 5e5 * 1.6e-4

    def reset():
        with torch.no_grad():
            m._xyz.copy_(saved)

    arms = {"hip": lambda: mcmc.add_noise(m, 1.6e-4, z=z), "torch_bmm": lambda: torch_noise(m, z, step)}
    for fn in arms.values():
        reset()
        fn()
    res = alternate(arms, args.reps, dev, reset)
    res["floor_bytes"] = P * 4 * (3 + 4 + 3 + 1 + 3 + 3)  # xyz, quaternion, log-scale, opacity, z read; xyz written
    res["floor_us"] = res["floor_bytes"] / HBM * 1e6
    res["share_of_floor_call_level"] = round(res["floor_us"] / res["hip"]["median_us"], 4)
    res["speedup_over_torch"] = round(res["torch_bmm"]["median_us"] / res["hip"]["median_us"], 2)
    return res


def case_densify(P, args, dev):
    """densify_and_prune on the scene of tools/densify_time.py, for scale (it changes P: a fresh copy per window, outside it)"""
    from goi_hyperplane_amd import densify
    from tools import densify_time as dt
    base = dt.model(P, dev)
    densify.densify_and_prune(dt.clone_model(base), 2e-4, 0.1, 4.0, None)
    return dt.timed(lambda mm: densify.densify_and_prune(mm, 2e-4, 0.1, 4.0, None), args.reps, dev, lambda: dt.clone_model(base))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--shares", default="0.01,0.05,0.5")
    ap.add_argument("--skip-densify", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_time.py measures the GPU and found none")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(dev), "P": args.P, "reps": args.reps, "hbm_bytes_per_s": HBM,
           "method": "device events around whole calls, arms alternating; medians and quartiles; kernel times not measured",
           "relocate": [case_relocate(args.P, float(s), args, dev) for s in args.shares.split(",")],
           "add_noise": case_noise(args.P, args, dev)}
    if not args.skip_densify:
        res["densify_and_prune_for_scale"] = case_densify(args.P, args, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
