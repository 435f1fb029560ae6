"""Times the neighbour-consistency loss and feature diffusion (goi_hyperplane_amd.smooth, csrc/smooth.hip) and
writes profiles/smooth.json.

    Cloud: the 1 M-point clustered cloud of tools/knn_time.py, features [P, 16], graphs of k = 3, 8, 16 from knn.graph.
    ALTERNATING in one process, per k: transpose; loss with gradient (forward + backward: the gradient is formed by the forward,
    the backward is one multiply); loss without gradient; one diffuse step; and THE YARDSTICK a user without this package has --
    the same loss and gradient restated in torch (index_select for both ends of every edge, index_add_ for the gradient, which
    uses float atomics and is not reproducible) on the same device.
    Floor: the compulsory traffic of a loss with gradient -- every row of f once as itself, once per out-edge and once per
    in-edge, idx, in_ptr and in_edge once, the gradient written -- over the streaming figure README.md measures the device by.

A window is two device events around one call and ends in a synchronise; per form the median, quartiles, extremes and the
medians of the two halves of the windows.  Needs a GPU.

    python tools/smooth_time.py [--out profiles/smooth.json] [--reps 20] [--points 1000000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tools.contrib_time import alternate  # noqa: E402
from tools.knn_time import STREAM_TBS, cloud  # noqa: E402

S = 16


def torch_loss(f, i, j, n_edges):
    """the same loss over the edge list (i -> j), unit weights; autograd's backward of the two index_selects is index_add_"""
    d = f.index_select(0, i) - f.index_select(0, j)
    return (d * d).sum() / n_edges


def floor_bytes(P, k, edges, grad):
    rows = P + edges + (edges if grad else 0)          # f: self, once per out-edge, once per in-edge
    b = rows * S * 4 + P * k * 4                       # ... and idx
    if grad:
        b += (P + 1) * 4 + P * k * 4 + P * S * 4       # in_ptr, in_edge, the gradient written
    return b


def row(x, k, reps):
    from goi_hyperplane_amd import knn, smooth
    P = int(x.shape[0])
    dev = x.device
    torch.manual_seed(k)
    f = torch.randn(P, S, device=dev, requires_grad=True)
    plain = f.detach()
    idx, _ = knn.graph(x, k)
    T = smooth.transpose(idx)
    edges = int(T[0][-1])
    keep = (idx >= 0).reshape(-1)
    i = torch.arange(P, device=dev).repeat_interleave(k)[keep]
    j = idx.reshape(-1)[keep].long()

    def ours_grad():
        f.grad = None
        smooth.loss(f, idx, transposed=T).backward()

    def torch_grad():
        f.grad = None
        torch_loss(f, i, j, edges).backward()

    nothing = lambda: None  # noqa: E731
    forms = {"transpose": (nothing, lambda: smooth.transpose(idx)),
             "loss_with_gradient": (nothing, ours_grad),
             "loss_without_gradient": (nothing, lambda: smooth.loss(plain, idx)),
             "diffuse_step": (nothing, lambda: smooth.diffuse(plain, idx)),
             "torch_loss_with_gradient": (nothing, torch_grad),
             "torch_loss_without_gradient": (nothing, lambda: torch_loss(plain, i, j, edges))}
    res = alternate(forms, reps)
    med = {n: r["median_ms"] for n, r in res.items()}
    # outside the windows: the two agree (the torch form sums in another order and with atomics)
    ours_grad()
    g_ours = f.grad.clone()
    torch_grad()
    out = {"P": P, "S": S, "k": k, "edges": edges, "max_in_degree": int((T[0][1:] - T[0][:-1]).max()), "windows": res,
           "torch_over_ours_with_gradient": round(med["torch_loss_with_gradient"] / med["loss_with_gradient"], 2),
           "torch_over_ours_without_gradient": round(med["torch_loss_without_gradient"] / med["loss_without_gradient"], 2),
           "max_abs_gradient_difference_to_torch": float((g_ours - f.grad).abs().max()), "floor": {}}
    for name, grad in (("loss_with_gradient", True), ("loss_without_gradient", False)):
        b = floor_bytes(P, k, edges, grad)
        floor_ms = b / (STREAM_TBS * 1e12) * 1e3
        out["floor"][name] = {"compulsory_bytes": b, "floor_ms": round(floor_ms, 4), "share_of_streaming": round(floor_ms / med[name], 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1_000_000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/smooth_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _lib
    _lib.load()
    doc = {"what": "neighbour-consistency loss, its gradient, the graph transpose and one diffusion step (goi_hyperplane_amd.smooth) next "
                   "to the same loss and gradient restated in torch (index_select / index_add_) on the clustered cloud of "
                   "tools/knn_time.py; tools/smooth_time.py",
           "device": torch.cuda.get_device_name(dev),
           "statistic": "two device events around one call, the window ending in a synchronise; forms alternate in one process after "
                        "warm-up; median, quartiles, extremes, medians of the two halves",
           "streaming_TB_per_s": STREAM_TBS, "rows": []}
    x = torch.from_numpy(cloud()[:args.points]).to(dev).contiguous()
    for k in (3, 8, 16):
        r = row(x, k, args.reps)
        print(json.dumps(r), flush=True)
        doc["rows"].append(r)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
