"""Times the photometric loss of train.py:137-140 and writes profiles/photometric.json.

    (a) loss fused: photometric.photometric_loss(image, gt) forward + backward (csrc/photometric.hip) against the
        reference's loss_utils restated -- l1_loss + ssim through five grouped 11x11 F.conv2d -- with torch autograd, on
        [3, H, W] fp32 images at 1600x1056 and 800x528; forward only and forward + backward.  The bytes each fused
        pass must move and the HBM-bound time they set (6.3 TB/s) are reported beside the measured time.
    (b) one RGB training iteration: render -> loss against a fixed target image -> backward -> FusedAdam over the
        Gaussian groups, with either loss.
Device events around --reps calls after --warmup, median and min over --rounds rounds, both arms alternated in one
process on the same seeded data.  The per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of
--only-fused.

    python tools/photometric_time.py [--out profiles/photometric.json] [--reps 50] [--rounds 5]
    python tools/photometric_time.py --only-fused --reps 20 --rounds 1        (the driver of the rocprofv3 run)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM = 6.3e12  # bytes/s, measured float4 copy rate of the MI355X


def window(dev):
    import math
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().to(dev).expand(3, 1, 11, 11).contiguous()


def torch_loss(image, gt, w, lam=0.2):
    """loss_utils.l1_loss / ssim as train.py:137-140 combines them"""
    conv = lambda t: torch.nn.functional.conv2d(t, w, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(image), conv(gt)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11, s22, s12 = conv(image * image) - mu1_sq, conv(gt * gt) - mu2_sq, conv(image * gt) - mu1_mu2
    m = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s11 + s22 + 0.03 ** 2))
    return (1.0 - lam) * torch.abs(image - gt).mean() + lam * (1.0 - m.mean())


def fused_loss(image, gt, _w):
    from goi_hyperplane_amd import photometric
    return photometric.photometric_loss(image, gt)[0]


def time_events(fn, reps, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def fused_bytes(H, W, C=3):
    """what the fused passes must move at least (fp32): forward reads x, y and writes 3 partial maps (image gradient
    only); backward reads the 3 maps, x, y and writes dx; the halo re-reads and block partials are not counted"""
    px = C * H * W
    return {"forward": 4 * px * (2 + 3), "backward": 4 * px * (3 + 2 + 1)}


def loss_case(H, W, args, dev, arms):
    g = torch.Generator(device=dev).manual_seed(H)
    gt = torch.rand(3, H, W, device=dev, generator=g)
    image = (gt + 0.1 * torch.randn(3, H, W, device=dev, generator=g)).clamp(0, 1).requires_grad_(True)
    w = window(dev)
    out = {}
    for name, fn in arms.items():
        fwd = lambda: fn(image, gt, w)  # noqa: E731

        def step():
            fn(image, gt, w).backward()
            image.grad = None

        for _ in range(args.warmup):
            step()
        out[name] = {"forward_us": [], "forward_backward_us": []}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            def fwd(fn=fn):
                with torch.no_grad():
                    fn(image, gt, w)

            def step(fn=fn):
                fn(image, gt, w).backward()
                image.grad = None

            out[name]["forward_us"].append(time_events(fwd, args.reps, dev))
            out[name]["forward_backward_us"].append(time_events(step, args.reps, dev))
    res = {"shape": [3, H, W]}
    for name, d in out.items():
        res[name] = {k: {"median": statistics.median(v), "min": min(v)} for k, v in d.items()}
    if "fused" in arms and "torch" in arms:
        res["speedup_forward_backward"] = (res["torch"]["forward_backward_us"]["median"] /
                                           res["fused"]["forward_backward_us"]["median"])
        res["max_abs_diff_loss"] = float((fused_loss(image, gt, w) - torch_loss(image, gt, w)).abs())
    nb = fused_bytes(H, W)
    res["fused_min_bytes"] = nb
    res["fused_hbm_bound_us"] = {k: v / HBM * 1e6 for k, v in nb.items()}
    return res


def train_iteration(args, dev, arms):
    from goi_hyperplane_amd.optim import FusedAdam
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import make_camera, make_scene
    sc = make_scene(args.gaussians, S=16, sh_degree=3, seed=0, log_scale_mean=-3.2)
    cam = TorchCamera(make_camera(1600, 1056, yaw=0.1), dev)
    bg = torch.zeros(3, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    gt = torch.rand(3, 1056, 1600, device=dev, generator=g)
    w = window(dev)
    res = {"gaussians": args.gaussians, "image": [3, 1056, 1600]}
    for name, fn in arms.items():
        pc = GaussianSet.from_scene(sc, dev)
        pc._semantics.requires_grad_(False)
        groups = [{"params": [p], "lr": 1e-4, "name": n} for n, p in pc.named_parameters() if p.requires_grad]
        opt = FusedAdam(groups, lr=0.0, eps=1e-15)

        def it():
            image = render(cam, pc, PipelineParams(), bg)["render"]
            fn(image, gt, w).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)

        for _ in range(args.warmup):
            it()
        ts = [time_events(it, max(args.reps // 5, 2), dev) for _ in range(args.rounds)]
        res[name] = {"iteration_us": {"median": statistics.median(ts), "min": min(ts)}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--only-fused", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_time.py measures the GPU and found none")
    dev = torch.device("cuda")
    arms = {"fused": fused_loss} if args.only_fused else {"fused": fused_loss, "torch": torch_loss}
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "rounds": args.rounds,
           "loss": [loss_case(H, W, args, dev, arms) for H, W in ((1056, 1600), (528, 800))],
           "train_iteration": train_iteration(args, dev, arms)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
