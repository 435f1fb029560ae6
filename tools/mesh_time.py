"""Times the mesh clean-up (goi_hyperplane_amd/mesh.py, csrc/mesh.hip) on the raw iso-surface of tools/field_time.py's
1 M-Gaussian scene at R = 128 and R = 256 and writes profiles/mesh.json.  Per stage -- components, clean (min_faces 64,
min_diag 0.2), decimate(target_faces=50000) of the cleaned mesh, vertex_normals, and the whole tail of mesh.extract behind
field.extract_mesh (clean -> decimate -> normals) -- three figures:

    device   the stage on the device, its read-backs included: median (min, max) over --rounds of windows of --iters calls
             between two device events, the stages ALTERNATING inside a round, after one warm-up round
    host     the route a user has without this module: the mesh copied to the host and the numpy restatement of
             tests/mesh_reference.py (components: scipy.sparse.csgraph.connected_components); wall clock, best of --host-runs
    torch    a restatement in torch on the same device where one exists -- normals with index_add_ (float atomics: not
             reproducible), clustering with torch.unique + index_add_ at the divisions the device chose (no bisection, no
             face dedup: less work); device events like the device figure

and for the stages a radix sort dominates, the traffic of its passes (16 bytes per pair and 8-bit pass) over the stage's time.

    python tools/mesh_time.py [--out profiles/mesh.json] [--rounds 5] [--iters 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import field_time  # noqa: E402

P, NUM_BLOCKS, RELAX = 1_000_000, 16, 1.5
TARGET = 50000


def torch_normals(v, f):
    i = f.long()
    a, b, c = v[i[:, 0]], v[i[:, 1]], v[i[:, 2]]
    fn = torch.linalg.cross(b - a, c - a)
    vn = torch.zeros_like(v)
    for k in range(3):
        vn.index_add_(0, i[:, k], fn)
    dot = (vn * vn).sum(-1, keepdim=True)
    vn = torch.where(dot > 1e-20, vn, torch.tensor([0.0, 0.0, 1.0], device=v.device))
    return vn / torch.sqrt(torch.clamp((vn * vn).sum(-1, keepdim=True), min=1e-20))


def torch_cluster(v, f, n):
    lo = v.amin(0)
    cell = (v.amax(0) - lo).max() / n
    q = torch.clamp(torch.floor((v - lo) / cell), max=n - 1).long()
    key = (q[:, 0] * n + q[:, 1]) * n + q[:, 2]
    uniq, inv = torch.unique(key, return_inverse=True)
    s = torch.zeros((uniq.numel(), 3), dtype=torch.float64, device=v.device).index_add_(0, inv, v.double())
    cnt = torch.zeros(uniq.numel(), dtype=torch.float64, device=v.device).index_add_(0, inv, torch.ones_like(inv, dtype=torch.float64))
    g = inv[f.long()]
    keep = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    return (s / cnt[:, None]).float(), g[keep]


def host_seconds(fn, runs):
    best = None
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best


def sort_passes(limit):
    return (max(1, int(limit).bit_length()) + 7) // 8


def measure(args, dev):
    from goi_hyperplane_amd import _lib, field, mesh
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from tests import mesh_reference as ref
    _lib.load()
    m = field_time.model(P, dev)
    pc = field_time.Stub(m)
    rows = []
    for R in args.resolutions:
        base = (m["xyz"], m["opacity"], m["scaling"], m["rotation"], R, NUM_BLOCKS, RELAX)
        f = field.density_grid(*base)
        thresh = float(torch.quantile(f.occ.reshape(-1)[:: max(1, R ** 3 // 1_000_000)], 0.9))  # field_time.py's surface
        raw = field.extract_mesh(pc, thresh, R, NUM_BLOCKS, RELAX, colors=m["rgb"])
        v, fa, c = raw.vertices, raw.faces, raw.colors
        V, F = int(v.shape[0]), int(fa.shape[0])
        cl = mesh.clean(v, fa, c)
        dec = mesh.decimate(cl.vertices, cl.faces, cl.colors, target_faces=TARGET)
        comp = mesh.components(fa, V)
        mesh.check_status(comp.status)

        def tail():
            a = mesh.clean(v, fa, c)
            b = mesh.decimate(a.vertices, a.faces, a.colors, target_faces=TARGET)
            return mesh.vertex_normals(b.vertices, b.faces)
        device = {
            "components": lambda: mesh.components(fa, V),
            "clean": lambda: mesh.clean(v, fa, c),
            "decimate": lambda: mesh.decimate(cl.vertices, cl.faces, cl.colors, target_faces=TARGET),
            "vertex_normals": lambda: mesh.vertex_normals(v, fa),
            "tail": tail,
            "torch_vertex_normals": lambda: torch_normals(v, fa),
            "torch_decimate": lambda: torch_cluster(cl.vertices, cl.faces, dec.divisions),
        }
        times = {k: [] for k in device}
        for r in range(args.rounds + 1):
            for name, fn in device.items():
                ms = field_time.window_ms(fn, args.iters)
                if r:
                    times[name].append(ms)

        def host_components():
            h = fa.cpu().numpy().astype(np.int64)
            i, j = np.concatenate([h[:, 0], h[:, 0]]), np.concatenate([h[:, 1], h[:, 2]])
            return connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(V, V)), directed=False)

        def host_tail():
            a = ref.clean(v.cpu().numpy(), fa.cpu().numpy(), c.cpu().numpy())
            b = ref.decimate(a[0], a[1], a[2], target_faces=TARGET)
            return ref.vertex_normals(b[0], b[1])
        hcl = [t.cpu().numpy() for t in (cl.vertices, cl.faces, cl.colors)]
        host = {
            "components": host_components,
            "clean": lambda: ref.clean(v.cpu().numpy(), fa.cpu().numpy(), c.cpu().numpy()),
            "decimate": lambda: ref.decimate(cl.vertices.cpu().numpy(), cl.faces.cpu().numpy(), cl.colors.cpu().numpy(),
                                             target_faces=TARGET),
            "vertex_normals": lambda: ref.vertex_normals(v.cpu().numpy(), fa.cpu().numpy()),
            "tail": host_tail,
        }
        row = {"P": P, "R": R, "density_thresh": round(thresh, 4), "vertices": V, "faces": F,
               "components": int((comp.vertex_label == torch.arange(V, device=dev, dtype=torch.int32)).sum()),
               "clean_vertices": int(cl.vertices.shape[0]), "clean_faces": int(cl.faces.shape[0]),
               "decimate_divisions": dec.divisions, "decimate_vertices": int(dec.vertices.shape[0]),
               "decimate_faces": int(dec.faces.shape[0])}
        for name, ts in times.items():
            row[name + "_ms"] = round(statistics.median(ts), 3)
            row[name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
        for name, fn in host.items():
            row["host_" + name + "_ms"] = round(1e3 * host_seconds(fn, args.host_runs), 1)
        # the traffic of the radix passes alone over the whole stage's time: a lower bound on what the sorts achieve
        nbytes = 16 * 3 * F * sort_passes(V)
        row["vertex_normals_sort_bytes"], row["vertex_normals_sort_gb_per_s"] = nbytes, round(nbytes / row["vertex_normals_ms"] / 1e6, 1)
        nbytes = 16 * F * sort_passes(V) * 3
        row["clean_sort_bytes"], row["clean_sort_gb_per_s"] = nbytes, round(nbytes / row["clean_ms"] / 1e6, 1)
        same = ref.vertex_normals(hcl[0], hcl[1])
        got = mesh.vertex_normals(cl.vertices, cl.faces).cpu().numpy()
        row["normals_bit_equal_to_restatement"] = bool(np.array_equal(same.view(np.int32), got.view(np.int32)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {
        "what": "mesh clean-up: csrc/mesh.hip against the numpy / scipy restatement on the host (copy included) and torch on the "
                "same device; tools/mesh_time.py",
        "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "iters_per_window": args.iters,
        "host_runs": args.host_runs,
        "statistic": "device and torch: median (and min, max) over the rounds of a window's time per call by device events, stages "
                     "alternating inside a round, one warm-up round; host: wall clock, best of host_runs",
        "rows": rows,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_time.py needs a ROCm device: a time taken anywhere else says nothing")
    doc = measure(args, torch.device("cuda:0"))
    print(json.dumps(doc, indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
