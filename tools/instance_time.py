"""Times the member lists and the per-instance statistics (goi_hyperplane_amd.instance, csrc/instance.hip) and
writes profiles/instance.json.

    Inputs, 1 M rows each, 16 channels, a positive weight and a hit byte per row:
      typical        the clustered cloud of tools/segment_time.py through segment.instances (k = 8, tau = 0.48): tens of
                     thousands of instances of some twenty rows;
      every_edge     the same cloud with every edge joining: ONE component of most rows beside the small ones -- the worst
                     case for a segmented reduction that gives an instance to one group of lanes;
      uniform_cube   1 M points uniform in the unit cube, every edge joining: one component of (nearly) all rows.
    ALTERNATING in one process, per input: members; stats (features, weight and hit, over those members); select end to end
    (members + stats + vote + rows_of); and THE OTHER ROUTE -- the same statistics restated in torch on the same device:
    index_add_ for the counts and sums (float atomics: other bits on every call), scatter_reduce_ amin / amax for the box.
    Floor: the compulsory traffic of stats -- every member id once, every member's position, feature row, weight and hit byte
    once, member_ptr and the outputs -- over the streaming figure README.md measures the device by.

A window is two device events around one call and ends in a synchronise; per form the median, quartiles, extremes and the
medians of the two halves of the windows.  Needs a GPU.

    python tools/instance_time.py [--out profiles/instance.json] [--reps 10] [--points 1000000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tools.contrib_time import alternate  # noqa: E402
from tools.knn_time import STREAM_TBS  # noqa: E402
from tools.segment_time import S, TAU, cloud_and_features  # noqa: E402


def torch_stats(label, K, xyz, f, w, hit):
    """the same statistics in torch: a row outside [0, K) goes to a slot K that is dropped; sums by index_add_, the box by
    scatter_reduce_.  Positions are summed as they are (float32, no pivot): it is the restatement a user would write."""
    P = label.shape[0]
    dev = label.device
    slot = torch.where((label >= 0) & (label < K), label, torch.full_like(label, K)).long()
    n = torch.zeros(K + 1, dtype=torch.int32, device=dev).index_add_(0, slot, torch.ones(P, dtype=torch.int32, device=dev))
    bits = ((hit[:, None] >> torch.arange(8, device=dev, dtype=torch.uint8)[None]) & 1).to(torch.int32)
    hits = torch.zeros((K + 1, 8), dtype=torch.int32, device=dev).index_add_(0, slot, bits)
    wsum = torch.zeros(K + 1, device=dev).index_add_(0, slot, w)
    sx = torch.zeros((K + 1, 3), device=dev).index_add_(0, slot, w[:, None] * xyz)
    outer = torch.stack([xyz[:, 0] * xyz[:, 0], xyz[:, 0] * xyz[:, 1], xyz[:, 0] * xyz[:, 2], xyz[:, 1] * xyz[:, 1],
                         xyz[:, 1] * xyz[:, 2], xyz[:, 2] * xyz[:, 2]], 1)
    sxx = torch.zeros((K + 1, 6), device=dev).index_add_(0, slot, w[:, None] * outer)
    sf = torch.zeros((K + 1, f.shape[1]), device=dev).index_add_(0, slot, w[:, None] * f)
    index = slot[:, None].expand(P, 3)
    lo = torch.full((K + 1, 3), float("inf"), device=dev).scatter_reduce_(0, index, xyz, "amin")
    hi = torch.full((K + 1, 3), float("-inf"), device=dev).scatter_reduce_(0, index, xyz, "amax")
    W = wsum[:, None].clamp_min(1e-30)
    c = sx / W
    cc = torch.stack([c[:, 0] * c[:, 0], c[:, 0] * c[:, 1], c[:, 0] * c[:, 2], c[:, 1] * c[:, 1], c[:, 1] * c[:, 2], c[:, 2] * c[:, 2]], 1)
    return n[:K], hits[:K], wsum[:K], c[:K], lo[:K], hi[:K], (sxx / W - cc)[:K], (sf / W)[:K]


def stats_floor_bytes(rows_in, P, K):
    per_row = 4 + 12 + S * 4 + 4 + 1  # member id, position, feature row, weight, hit byte
    per_instance = 4 + 4 + 32 + 4 + 12 + 12 + 12 + 24 + S * 4  # member_ptr, n, hits, wsum, centroid, lo, hi, cov, feature
    return rows_in * per_row + K * per_instance


def row(name, label, K, xyz, f, reps):
    from goi_hyperplane_amd import instance
    P = int(label.shape[0])
    g = torch.Generator(device=label.device).manual_seed(11)
    w = 0.05 + torch.rand(P, device=label.device, generator=g)
    hit = torch.randint(0, 256, (P,), device=label.device, generator=g, dtype=torch.uint8)
    flag = hit > 127
    m = instance.members(label, K)
    nothing = lambda: None  # noqa: E731
    forms = {"members": (nothing, lambda: instance.members(label, K)),
             "stats": (nothing, lambda: instance.stats(label, xyz, f, w, hit, members=m)),
             "select": (nothing, lambda: instance.select(label, flag, 0.5, capacity=K)),
             "torch_stats": (nothing, lambda: torch_stats(label, K, xyz, f, w, hit))}
    res = alternate(forms, reps)
    med = {n: r["median_ms"] for n, r in res.items()}
    # outside the windows: the routes agree (integers exactly, floats to float32 summation noise), and a second call repeats
    st, again = instance.stats(label, xyz, f, w, hit, members=m), instance.stats(label, xyz, f, w, hit, members=m)
    t = torch_stats(label, K, xyz, f, w, hit)
    same_bits = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(st[:8], again[:8]))
    torch_repeats = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(t, torch_stats(label, K, xyz, f, w, hit)))
    rows_in = int(m.ptr[K].cpu())
    b = stats_floor_bytes(rows_in, P, K)
    floor_ms = b / (STREAM_TBS * 1e12) * 1e3
    return {"input": name, "P": P, "S": S, "K": K, "rows_in_an_instance": rows_in, "largest_instance": int(st.n.max().cpu()) if K else 0,
            "windows": res, "torch_stats_over_stats": round(med["torch_stats"] / med["stats"], 2),
            "counts_and_box_equal_torch": bool(torch.equal(st.n, t[0]) and torch.equal(st.hits, t[1]) and torch.equal(st.lo, t[4])
                                         and torch.equal(st.hi, t[5])),
            "largest_centroid_difference_from_torch": float((st.centroid - t[3]).abs().max().cpu()) if K else 0.0,
            "same_bits_on_a_second_call": same_bits, "torch_same_bits_on_a_second_call": torch_repeats,
            "stats_floor": {"compulsory_bytes": b, "floor_ms": round(floor_ms, 4), "share_of_streaming": round(floor_ms / med["stats"], 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=1_000_000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/instance_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _lib, knn, segment
    _lib.load()
    doc = {"what": "the member lists and the per-instance statistics (goi_hyperplane_amd.instance) next to the same statistics in torch "
                   "(index_add_, scatter_reduce_) on the same device, over the partitions of tools/segment_time.py; tools/instance_time.py",
           "device": torch.cuda.get_device_name(dev),
           "statistic": "two device events around one call, the window ending in a synchronise; forms alternate in one process after "
                        "warm-up; median, quartiles, extremes, medians of the two halves",
           "streaming_TB_per_s": STREAM_TBS, "rows": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            json.dump(doc, out, indent=1)

    xh, fh = cloud_and_features(args.points)
    x, f = torch.from_numpy(xh).to(dev).contiguous(), torch.from_numpy(fh).to(dev).contiguous()
    idx, _ = knn.graph(x, 8)
    g = torch.Generator(device=dev).manual_seed(7)
    cube = torch.rand((args.points, 3), device=dev, generator=g)
    inputs = (("typical", x, segment.components(idx, segment.edges(idx, f, TAU))), ("every_edge", x, segment.components(idx)),
              ("uniform_cube", cube, segment.components(knn.graph(cube, 8)[0])))
    for name, pos, seg in inputs:
        r = row(name, seg.label, int(seg.count.cpu()[0]), pos, f, args.reps)
        print(json.dumps(r), flush=True)
        doc["rows"].append(r)
        save()
    stats_ms = {r["input"]: r["windows"]["stats"]["median_ms"] for r in doc["rows"]}
    doc["one_component_over_typical_stats"] = {n: round(stats_ms[n] / stats_ms["typical"], 2) for n in ("every_edge", "uniform_cube")}
    print(json.dumps(doc["one_component_over_typical_stats"]), flush=True)
    save()


if __name__ == "__main__":
    main()
