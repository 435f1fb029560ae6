"""Times the mesh extraction (goi_hyperplane_amd/field.py, csrc/field.hip) on synthetic models resident on the device and
writes profiles/field.json:

    density_grid    the density grid alone (bounds, preparation, sort, the block kernel), with and without colour channels
    extract_mesh    density_grid + isosurface (its read-back of the two counts included) + the map to world coordinates
    torch           the block loop restated in torch on the same device (tests/field_reference.py:
                    density_torch_blockloop): one host iteration per block, [points, members, 3] and [points, members, 6]
                    tensors materialised, batches of 1024 Gaussians.  Where all blocks would take minutes it visits every
                    k-th block and the row says so: "torch_blocks_visited" of "torch_blocks", "torch_ms" for the visited
                    blocks alone and "torch_ms_all_blocks_extrapolated" scaled by the block count.

at 1 M and 100 k Gaussians, R = 128 and 256 (16 blocks per axis, relax 1.5).  The model: Gaussians on four noisy closed
surfaces (a scene's Gaussians sit on surfaces, not in a volume), log-normal scales about 0.4 % of the extent with anisotropy
up to 10 : 1, opacities uniform in (0, 1).  The device figures are medians over --rounds of windows of --iters calls
between two device events, the variants ALTERNATING inside a round, after one warm-up round.

    python tools/field_time.py [--out profiles/field.json] [--rounds 5] [--iters 2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SIZES = ((1_000_000, 128), (1_000_000, 256), (100_000, 128), (100_000, 256))
NUM_BLOCKS, RELAX = 16, 1.5


def model(P, dev):
    g = torch.Generator(device=dev).manual_seed(P)
    n = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    u = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    d = torch.nn.functional.normalize(n(P, 3), dim=1)
    which = torch.randint(0, 4, (P,), device=dev, generator=g)
    centers = torch.tensor([[0.0, 0.0, 0.0], [1.2, 0.3, -0.2], [-0.9, 0.8, 0.4], [0.2, -1.0, 0.6]], device=dev)[which]
    radii = torch.tensor([0.8, 0.45, 0.5, 0.35], device=dev)[which]
    xyz = centers + d * (radii * (1 + 0.02 * n(P)))[:, None] * torch.tensor([1.0, 0.8, 0.6], device=dev)
    smin = 0.012 * torch.exp(0.4 * n(P, 1))
    scaling = smin * (1 + 9 * u(P, 3))
    return dict(xyz=xyz.contiguous(), opacity=u(P), scaling=scaling.contiguous(), rotation=n(P, 4), rgb=u(P, 3))


class Stub:
    def __init__(self, m):
        self.get_xyz, self.get_opacity, self.get_scaling, self.get_rotation = m["xyz"], m["opacity"], m["scaling"], m["rotation"]
        self.rgb = m["rgb"]


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def measure(args, dev):
    from goi_hyperplane_amd import _lib, field
    from tests.field_reference import density_torch_blockloop
    _lib.load()
    rows = []
    models = {}
    for P, R in SIZES:
        if P not in models:
            models[P] = model(P, dev)
        m = models[P]
        pc = Stub(m)
        base = (m["xyz"], m["opacity"], m["scaling"], m["rotation"], R, NUM_BLOCKS, RELAX)
        f = field.density_grid(*base)
        thresh = float(torch.quantile(f.occ.reshape(-1)[:: max(1, R ** 3 // 1_000_000)], 0.9))  # a surface that exists
        variants = {
            "density_grid": lambda: field.density_grid(*base),
            "density_grid_rgb": lambda: field.density_grid(*base, attributes=m["rgb"]),
            "extract_mesh": lambda: field.extract_mesh(pc, thresh, R, NUM_BLOCKS, RELAX, colors=m["rgb"]),
        }
        stride = args.torch_stride_1m if P >= 1_000_000 else args.torch_stride_100k
        visited = []

        def torch_loop():
            visited.append(density_torch_blockloop(m["xyz"], m["opacity"], m["scaling"], m["rotation"], R, NUM_BLOCKS, RELAX,
                                                   block_stride=stride)[1])
        times = {k: [] for k in variants}
        for r in range(args.rounds + 1):
            for name, fn in variants.items():
                ms = window_ms(fn, args.iters)
                if r:
                    times[name].append(ms)
        mesh = field.extract_mesh(pc, thresh, R, NUM_BLOCKS, RELAX, colors=m["rgb"])
        row = {"P": P, "R": R, "num_blocks": NUM_BLOCKS, "relax_ratio": RELAX, "density_thresh": round(thresh, 4),
               "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0])}
        for name, ts in times.items():
            row[name + "_ms"] = round(statistics.median(ts), 3)
            row[name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
        ts = [window_ms(torch_loop, 1) for _ in range(args.torch_rounds + 1)][1:]
        row["torch_blocks"], row["torch_blocks_visited"] = NUM_BLOCKS ** 3, visited[-1]
        row["torch_ms"] = round(statistics.median(ts), 2)
        row["torch_ms_min_max"] = [round(min(ts), 2), round(max(ts), 2)]
        row["torch_ms_all_blocks_extrapolated"] = round(row["torch_ms"] * NUM_BLOCKS ** 3 / visited[-1], 1)
        if stride == 1:
            ref = density_torch_blockloop(m["xyz"], m["opacity"], m["scaling"], m["rotation"], R, NUM_BLOCKS, RELAX)[0]
            row["max_abs_difference_to_torch"] = float((ref - f.occ).abs().max())
            row["max_occ"] = float(ref.max())
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {
        "what": "mesh extraction: csrc/field.hip against the block loop restated in torch on the same device; tools/field_time.py",
        "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "iters_per_window": args.iters,
        "torch_rounds": args.torch_rounds,
        "statistic": "median (and min, max) over the rounds of a window's time per call by device events, variants alternating "
                     "inside a round, one warm-up round; the torch loop: windows of one call, one warm-up",
        "rows": rows,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--torch-stride-1m", type=int, default=61, help="the torch loop visits every k-th block at 1 M Gaussians")
    ap.add_argument("--torch-stride-100k", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/field_time.py needs a ROCm device: a time taken anywhere else says nothing")
    doc = measure(args, torch.device("cuda:0"))
    print(json.dumps(doc, indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
