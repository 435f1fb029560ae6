"""Times the edge gate and the connected components of the k-NN graph (goi_hyperplane_amd.segment, csrc/segment.hip; DESIGN.md
4.29) and writes profiles/segment.json.

    Cloud: the 1 M-point clustered cloud of tools/knn_time.py; features [P, 16] that follow its 2000 blobs (a vector per blob
    plus 0.1 noise), tau = 0.48; graphs of k = 3, 8, 16 from knn.graph (built outside the windows).
    ALTERNATING in one process, per k: edges; components (with that join); instances without the graph (= edges + components);
    and THE ONLY OTHER ROUTES -- the same gate restated in torch (index_select, subtract, square, sum, compare) on the same
    device, and the same partition by scipy.sparse.csgraph.connected_components on the host, the copies of idx and join to the
    host and of the labels back included.
    WORST CASE for the union-find and the size count: every edge joins.  On the clustered cloud (`components_every_edge`) and on
    1 M points uniform in a cube with k = 8, whose graph is one component of (nearly) all rows (`one_component`); the size of the
    largest component is recorded next to the time.
    Floor: the compulsory traffic of the gate -- idx once, every row of f once as itself and once per edge, join written -- over
    the streaming figure README.md measures the device by.

A window is two device events around one call and ends in a synchronise; per form the median, quartiles, extremes and the
medians of the two halves of the windows.  Needs a GPU.

    python tools/segment_time.py [--out profiles/segment.json] [--reps 10] [--points 1000000]
    python tools/segment_time.py --only typical | every_edge       (the driver of a rocprofv3 --kernel-trace --stats run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.contrib_time import alternate  # noqa: E402
from tools.knn_time import STREAM_TBS  # noqa: E402

S = 16
TAU = 0.48


def cloud_and_features(P):
    """tools/knn_time.py's cloud (the same draws), with the blob of every point kept for its features"""
    rng = np.random.default_rng(5)
    c = rng.standard_normal((2000, 3)) * 5
    which = rng.integers(0, 2000, 1_000_000)
    x = (c[which] + 0.3 * rng.standard_normal((1_000_000, 3))).astype(np.float32)
    frng = np.random.default_rng(6)
    f = (frng.standard_normal((2000, S))[which] + 0.1 * frng.standard_normal((1_000_000, S))).astype(np.float32)
    return x[:P], f[:P]


def torch_gate(f, idx, tau):
    """the same gate in torch: both ends of every edge by index_select, subtract, square, sum, compare"""
    P, k = idx.shape
    j = idx.clamp(min=0).reshape(-1).long()
    i = torch.arange(P, device=idx.device).repeat_interleave(k)
    d = f.index_select(0, i) - f.index_select(0, j)
    ok = ((d * d).sum(dim=1) <= tau).reshape(P, k)
    return (ok & (idx >= 0) & (idx != torch.arange(P, device=idx.device)[:, None])).to(torch.uint8)


def scipy_components(idx, join):
    """the same partition on the host: idx and join copied down, the labels copied back"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    P, k = idx.shape
    idx_h, join_h = idx.cpu().numpy(), join.cpu().numpy()
    i, m = np.nonzero(join_h)
    A = sp.coo_matrix((np.ones(len(i), np.int8), (i, idx_h[i, m])), shape=(P, P)).tocsr()
    n, lab = connected_components(A, directed=True, connection="weak")
    return n, torch.from_numpy(lab).to(idx.device)


def gate_floor_bytes(P, k, edges):
    return (P + edges) * S * 4 + P * k * 4 + P * k  # f: self and once per edge; idx; join written


def describe(seg):
    return {"components": int(seg.count.cpu()[0]), "largest_component": int(seg.size.max().cpu()), "status": int(seg.status.cpu()[0])}


def row(x, f, k, reps):
    from goi_hyperplane_amd import knn, segment
    P = int(x.shape[0])
    idx, dist2 = knn.graph(x, k)
    join = segment.edges(idx, f, TAU)
    nothing = lambda: None  # noqa: E731
    forms = {"edges": (nothing, lambda: segment.edges(idx, f, TAU)),
             "components": (nothing, lambda: segment.components(idx, join)),
             "instances_without_graph": (nothing, lambda: segment.components(idx, segment.edges(idx, f, TAU))),
             "components_every_edge": (nothing, lambda: segment.components(idx)),
             "torch_gate": (nothing, lambda: torch_gate(f, idx, TAU)),
             "scipy_components_host": (nothing, lambda: scipy_components(idx, join))}
    res = alternate(forms, reps)
    med = {n: r["median_ms"] for n, r in res.items()}
    # outside the windows: the routes agree
    seg = segment.components(idx, join)
    n_host, lab = scipy_components(idx, join)
    pairs = torch.unique(lab.long() * (P + 1) + seg.root.long()).numel()  # one (host label, root) pair per component on both sides
    same_partition = pairs == n_host == torch.unique(seg.root).numel()
    gate_differs = int((torch_gate(f, idx, TAU) != join).sum())  # (torch sums in another order: entries within an ulp of tau may differ)
    edges = int(((idx >= 0) & (idx < P)).sum())
    b = gate_floor_bytes(P, k, edges)
    floor_ms = b / (STREAM_TBS * 1e12) * 1e3
    return {"P": P, "S": S, "k": k, "tau": TAU, "edges": edges, "joining_edges": int(join.sum()), "typical": describe(seg),
            "every_edge": describe(segment.components(idx)), "scipy_components": n_host, "same_partition_as_scipy": same_partition,
            "gate_entries_that_differ_from_torch": gate_differs, "windows": res,
            "torch_gate_over_edges": round(med["torch_gate"] / med["edges"], 2),
            "scipy_host_over_components": round(med["scipy_components_host"] / med["components"], 2),
            "every_edge_over_typical_components": round(med["components_every_edge"] / med["components"], 2),
            "gate_floor": {"compulsory_bytes": b, "floor_ms": round(floor_ms, 4), "share_of_streaming": round(floor_ms / med["edges"], 4)}}


def one_component(P, k, reps, dev):
    """every edge of the k-NN graph of P points uniform in a cube joins: one component of (nearly) all rows"""
    from goi_hyperplane_amd import knn, segment
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand((P, 3), device=dev, generator=g)
    idx, _ = knn.graph(x, k)
    res = alternate({"components_every_edge": (lambda: None, lambda: segment.components(idx))}, reps)
    return {"P": P, "k": k, "cloud": "uniform in the unit cube", **describe(segment.components(idx)), "windows": res}


def only(which, points, k, dev, calls=10):
    """the driver of a `rocprofv3 --kernel-trace --stats` run of its own (per-kernel times): `calls` instances-without-graph calls
    at one k, `typical` through the gate or `every_edge` without a join"""
    from goi_hyperplane_amd import knn, segment
    xh, fh = cloud_and_features(points)
    x, f = torch.from_numpy(xh).to(dev).contiguous(), torch.from_numpy(fh).to(dev).contiguous()
    idx, _ = knn.graph(x, k)
    for _ in range(calls):
        seg = segment.components(idx, segment.edges(idx, f, TAU)) if which == "typical" else segment.components(idx)
        torch.cuda.synchronize()
    print(which, describe(seg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--only", choices=("typical", "every_edge"), help="k = 8 calls only, no windows (for the rocprofv3 kernel split)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/segment_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _lib
    _lib.load()
    if args.only:
        return only(args.only, args.points, 8, dev)
    doc = {"what": "the feature-gated edges and the connected components of the k-NN graph (goi_hyperplane_amd.segment) next to the same "
                   "gate in torch on the same device and the same partition by scipy.sparse.csgraph.connected_components on the host, on "
                   "the clustered cloud of tools/knn_time.py; tools/segment_time.py",
           "device": torch.cuda.get_device_name(dev),
           "statistic": "two device events around one call, the window ending in a synchronise; forms alternate in one process after "
                        "warm-up; median, quartiles, extremes, medians of the two halves",
           "streaming_TB_per_s": STREAM_TBS, "rows": []}
    xh, fh = cloud_and_features(args.points)
    x, f = torch.from_numpy(xh).to(dev).contiguous(), torch.from_numpy(fh).to(dev).contiguous()

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            json.dump(doc, out, indent=1)

    for k in (3, 8, 16):
        r = row(x, f, k, args.reps)
        print(json.dumps(r), flush=True)
        doc["rows"].append(r)
        save()
    doc["one_component"] = one_component(args.points, 8, args.reps, dev)
    print(json.dumps(doc["one_component"]), flush=True)
    save()


if __name__ == "__main__":
    main()
