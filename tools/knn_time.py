"""Times the k-NN graph (goi_knn_graph, goi_hyperplane_amd.knn) next to distCUDA2 and writes
profiles/knn_graph.json.

    (a) the 1 M-point clustered cloud of tests/test_gpu_knn.py::test_scene_scale_cloud_against_oracle and its first 100 k points.
        ALTERNATING in one process: distCUDA2; knn.graph at k = 3, 8, 16; a knn.query of ONE point against the cloud at k = 8
        (the references' whole preparation -- bounds, Morton codes, sort, boxes -- and next to no search: what it costs is what
        a graph call spends outside knn_graph_k); knn.complete_labels at k = 8 with 24 % of the points labelled.
        search = graph - preparation; its compulsory traffic is 16 bytes read and 8 k bytes written per query.
    (b) the yardstick a user without this package has: blocked torch.cdist + topk(k + 1, smallest) on the same device.  At 100 k
        points every query block is run; at 1 M a SAMPLE of query blocks is timed and multiplied up to all of them (stated in
        the output as "extrapolated").

A window is two device events around one call and ends in a synchronise; per form the median, quartiles, extremes and the
medians of the two halves of the windows.  Needs a GPU.

    python tools/knn_time.py [--out profiles/knn_graph.json] [--reps 20]
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

STREAM_TBS = 6.29  # the streaming figure README.md measures the device by


def cloud():
    rng = np.random.default_rng(5)
    c = rng.standard_normal((2000, 3)) * 5
    return (c[rng.integers(0, 2000, 1_000_000)] + 0.3 * rng.standard_normal((1_000_000, 3))).astype(np.float32)


def cdist_topk(x, k, block, blocks=None):
    """the k nearest others by dense distance blocks; blocks: how many query blocks to run (None: all)"""
    n = (x.shape[0] + block - 1) // block
    for b in range(n if blocks is None else min(blocks, n)):
        q = x[b * block:(b + 1) * block]
        torch.cdist(q, x).topk(k + 1, dim=1, largest=False)
    return n


def rows(x, reps):
    from goi_hyperplane_amd import knn
    from simple_knn._C import distCUDA2
    P = int(x.shape[0])
    one = x[:1].contiguous()
    torch.manual_seed(1)
    labels = torch.where(torch.rand(P, device=x.device) < 0.24, torch.randint(0, 8, (P,), device=x.device), -1)
    nothing = lambda: None  # noqa: E731
    forms = {"distCUDA2": (nothing, lambda: distCUDA2(x)),
             "graph_k3": (nothing, lambda: knn.graph(x, 3)),
             "graph_k8": (nothing, lambda: knn.graph(x, 8)),
             "graph_k16": (nothing, lambda: knn.graph(x, 16)),
             "preparation_one_query_k8": (nothing, lambda: knn.query(one, x, 8)),
             "complete_labels_k8_24pct_labelled": (nothing, lambda: knn.complete_labels(x, labels, k=8))}
    res = alternate(forms, reps)
    med = {n: r["median_ms"] for n, r in res.items()}
    prep = med["preparation_one_query_k8"]
    row = {"P": P, "labelled": int((labels >= 0).sum()), "windows": res, "graph_k3_over_distCUDA2": round(med["graph_k3"] / med["distCUDA2"], 3),
           "search_ms": {}, "search_compulsory_TB_per_s": {}, "search_share_of_streaming": {}}
    for k in (3, 8, 16):
        ms = med[f"graph_k{k}"] - prep
        tbs = P * (16 + 8 * k) / (ms * 1e-3) / 1e12
        row["search_ms"][f"k{k}"] = round(ms, 4)
        row["search_compulsory_TB_per_s"][f"k{k}"] = round(tbs, 4)
        row["search_share_of_streaming"][f"k{k}"] = round(tbs / STREAM_TBS, 4)
    # the graph's first three distances ARE distCUDA2's: checked here once, outside the windows
    d = knn.graph(x, 3)[1]
    # (divided by a TENSOR of threes: torch turns a division by a Python scalar into a multiplication by its reciprocal)
    mean = torch.div((d[:, 0] + d[:, 1]) + d[:, 2], torch.full_like(d[:, 0], 3.0))
    row["graph_k3_reproduces_distCUDA2_bitwise"] = bool(torch.equal(mean, distCUDA2(x)))
    return row, med


def yardstick(x, med, reps):
    P = int(x.shape[0])
    block = 4096 if P <= 200_000 else 1024
    n = (P + block - 1) // block
    sample = None if P <= 200_000 else 8
    out = {"P": P, "query_block": block, "query_blocks": n, "blocks_timed": n if sample is None else sample,
           "extrapolated": sample is not None}
    for k in (3, 8, 16):
        r = alternate({"cdist_topk": (lambda: None, lambda k=k: cdist_topk(x, k, block, sample))}, max(reps // 4, 5), warmup=1)["cdist_topk"]
        scale = 1.0 if sample is None else n / sample
        out[f"k{k}"] = {"windows": r, "whole_cloud_ms": round(r["median_ms"] * scale, 3),
                        "over_graph": round(r["median_ms"] * scale / med[f"graph_k{k}"], 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_graph.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/knn_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _lib
    _lib.load()
    doc = {"what": "exact k-NN graph (knn.graph, knn.complete_labels) next to distCUDA2 and to blocked torch.cdist + topk on the clustered "
                   "cloud of test_scene_scale_cloud_against_oracle; tools/knn_time.py",
           "device": torch.cuda.get_device_name(dev),
           "statistic": "two device events around one call, the window ending in a synchronise; forms alternate in one process after "
                        "warm-up; median, quartiles, extremes, medians of the two halves",
           "streaming_TB_per_s": STREAM_TBS, "clouds": [], "cdist_topk": []}
    pts = torch.from_numpy(cloud()).to(dev)
    for P in (100_000, 1_000_000):
        x = pts[:P].contiguous()
        row, med = rows(x, args.reps)
        print(json.dumps(row), flush=True)
        doc["clouds"].append(row)
        y = yardstick(x, med, args.reps)
        print(json.dumps(y), flush=True)
        doc["cdist_topk"].append(y)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
