"""Times the exact DBSCAN (cluster.dbscan, csrc/dbscan.hip) against sklearn.cluster.DBSCAN on the same host, and
semantic.group_points (gui/main.py:1595-1665) end to end, and writes profiles/dbscan.json.

Inputs: clustered sets with 10 % uniform noise at n = 100 k, 1 M, 3 M; the headline scene's means3D at 1 M
(scene.HEADLINE); one dense cell of duplicates (1 M copies of a point); uniformly sparse points (1 M in a 400^3 box).
Parameters eps 0.35 with min_samples 600 and 10.  GPU: device events around the call's launches (no host read-back
inside them), median of --reps after one warm-up.  sklearn: wall seconds of fit() in a child process capped at --cap
seconds ("did not finish" otherwise).  group_points: 512x512, K blobs, geometry cache off and on, host clock around a
synchronisation.  The per-kernel split comes from a separate `rocprofv3 --kernel-trace --stats` run of --only-gpu.

    python tools/dbscan_time.py [--out profiles/dbscan.json] [--reps 5] [--cap 120] [--only-gpu] [--sizes 100000,...]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from goi_hyperplane_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")


def clustered(n, seed=0, centers=16, extent=6.0, spread=0.5, noise=0.1):
    rng = np.random.default_rng(seed)
    n_noise = int(n * noise)
    c = rng.uniform(-extent, extent, size=(centers, 3))
    which = rng.integers(0, centers, size=n - n_noise)
    pts = np.concatenate([c[which] + rng.normal(0.0, spread, size=(n - n_noise, 3)),
                          rng.uniform(-extent - 2, extent + 2, size=(n_noise, 3))])
    return pts[rng.permutation(n)].astype(np.float32)


def inputs(sizes):
    from goi_hyperplane_amd.scene import HEADLINE, make_scene
    out = {f"clustered_{n // 1000}k": clustered(n) for n in sizes}
    sc = make_scene(HEADLINE["P"], S=HEADLINE["S"], sh_degree=3, seed=0, extent=HEADLINE["extent"],
                    log_scale_mean=HEADLINE["log_scale_mean"], log_scale_std=HEADLINE["log_scale_std"])
    out["headline_means3D_1000k"] = np.ascontiguousarray(sc.means3D, dtype=np.float32)
    out["duplicates_1000k"] = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (1_000_000, 1))
    out["sparse_uniform_1000k"] = np.random.default_rng(1).uniform(-200, 200, size=(1_000_000, 3)).astype(np.float32)
    return out


def gpu_ms(x, eps, ms, reps):
    """Median device time of goi_semantic_dbscan's launches (events around the asynchronous call)."""
    import ctypes as C
    lib = _lib.load()
    n = x.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    result = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.goi_semantic_dbscan_workspace_bytes(n)), 1), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ts = []
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = lib.goi_semantic_dbscan(n, C.c_void_p(x.data_ptr()), eps, ms, C.c_void_p(labels.data_ptr()), None,
                                     C.c_void_p(result.data_ptr()), C.c_void_p(ws.data_ptr()), stream)
        b.record()
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        if r:
            ts.append(a.elapsed_time(b))
    k, flags = result.tolist()
    assert flags == 0, flags
    lab = labels.long()
    return statistics.median(ts), {"clusters": k, "noise": int((lab == -1).sum()), "ws_bytes": int(ws.numel())}


SK_CHILD = """
import resource, sys, time, numpy as np
resource.setrlimit(resource.RLIMIT_AS, (int(sys.argv[4]) << 30, int(sys.argv[4]) << 30))  # neighbourhood lists: cap, no OOM
from sklearn.cluster import DBSCAN
x = np.load(sys.argv[1]); t = time.perf_counter()
DBSCAN(eps=float(sys.argv[2]), min_samples=int(sys.argv[3])).fit(x)
print(time.perf_counter() - t)
"""


def sklearn_s(x, eps, ms, cap, mem_gb=24):
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "x.npy")
        np.save(f, x)
        try:
            r = subprocess.run([sys.executable, "-c", SK_CHILD, f, str(eps), str(ms), str(mem_gb)], capture_output=True, text=True,
                               timeout=cap)
        except subprocess.TimeoutExpired:
            return f"did not finish in {cap} s"
        if r.returncode != 0:
            return f"failed ({mem_gb} GB address-space cap): {r.stderr.strip().splitlines()[-1] if r.stderr.strip() else r.returncode}"
        return float(r.stdout.strip().splitlines()[-1])


def group_points_timing(K, reps):
    from goi_hyperplane_amd import rasterizer
    from goi_hyperplane_amd.render import GaussianSet, TorchCamera
    from goi_hyperplane_amd.scene import make_camera
    from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, group_points, svm_score_fn
    rng = np.random.default_rng(2)
    S, per = 16, 4000
    ang = np.linspace(0, 2 * np.pi, K, endpoint=False)
    centers = np.stack([1.6 * np.cos(ang), 1.2 * np.sin(ang), np.zeros(K)], 1)
    xyz = np.concatenate([c + rng.normal(0, 0.12, size=(per, 3)) for c in centers]).astype(np.float32)
    P = len(xyz)
    t = lambda v: torch.tensor(np.asarray(v, np.float32), device=dev)  # noqa: E731
    sem = np.zeros((P, S), np.float32)
    sem[:, 0] = 1
    shs = np.zeros((P, 16, 3), np.float32)
    shs[:, 0] = 0.5
    pc = GaussianSet(t(xyz), t(np.full((P, 3), 0.03)), t(np.tile([1.0, 0, 0, 0], (P, 1))), t(np.full((P, 1), 0.9)), t(shs),
                     t(sem))
    mlp = SemanticModel(dim_in=S, dim_out=4, num_layer=1, use_bias=True, device=dev)
    with torch.no_grad():
        mlp.layers[0].weight.zero_()
        mlp.layers[0].weight[0, 0] = 10
        mlp.layers[0].bias.copy_(torch.tensor([-1.0, 0, -5, -5]))
    u = torch.nn.functional.normalize(torch.randn(256, device=dev), dim=0)
    lut = torch.stack([u, -u, -u, -u])
    svm = LinearSVM().to(dev)
    svm.weight_set(u.reshape(1, -1))
    cam = TorchCamera(make_camera(512, 512), dev)
    bg = torch.zeros(3, device=dev)
    sel = torch.ones(P, dtype=torch.bool, device=dev)
    res = torch.zeros(512 * 512, dtype=torch.bool, device=dev)
    res[: 512 * 256] = True
    out = {}
    for cache in (False, True):
        rasterizer.set_geometry_cache((1 << 30) if cache else 0)
        ts = []
        for r in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = group_points(pc, sel, cam, bg, mlp, lut, svm_score_fn(svm), res, min_samples=600)
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
        out["cache_on" if cache else "cache_off"] = {"ms": statistics.median(ts), "kept": int(got.sum())}
    rasterizer.set_geometry_cache(0)
    out.update({"K": K, "P": P, "W": 512, "H": 512})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=120)
    ap.add_argument("--sizes", default="100000,1000000,3000000")
    ap.add_argument("--only-gpu", action="store_true", help="GPU runs only (for the rocprofv3 kernel split)")
    args = ap.parse_args()
    _lib.load()
    rows = []
    for name, x in inputs([int(s) for s in args.sizes.split(",")]).items():
        xt = torch.from_numpy(x).to(dev)
        for ms in (600, 10):
            t, info = gpu_ms(xt, 0.35, ms, args.reps)
            row = {"input": name, "n": int(x.shape[0]), "eps": 0.35, "min_samples": ms, "gpu_ms": round(t, 3), **info}
            if not args.only_gpu:
                row["sklearn_s"] = sklearn_s(x, 0.35, ms, args.cap)
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = {"what": "cluster.dbscan (csrc/dbscan.hip) vs sklearn.cluster.DBSCAN on the same host; tools/dbscan_time.py",
           "device": torch.cuda.get_device_name(dev), "host_cpus": os.cpu_count(), "rows": rows}
    if not args.only_gpu:
        doc["group_points"] = [group_points_timing(K, args.reps) for K in (4, 8)]
        print(json.dumps(doc["group_points"]), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
