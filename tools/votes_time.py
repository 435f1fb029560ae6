"""Times the blend-weight votes (goi_raster_contrib_votes, goi_hyperplane_amd.contrib) and writes
profiles/votes.json.

    (a) the kernel: the headline scene (1 M Gaussians), 1600 x 1056, first orbit camera.  One exact forward; then, ALTERNATING in
        one process, each into a zeroed array: the votes of that frame under four label maps -- uniform, a slanted half-plane and
        a 1-pixel checkerboard with K = 2, and 64 distinct labels per quadrant with K = 64 -- next to contrib_k's peak into zeros
        (goi_raster_contrib_frame) and to the only other route to such sums: a trainable forward plus the backward of
        `semantics` alone with a one-hot upstream for the same K = 2 labels (K = 64 would take 64 / S such passes).  The count
        of atomics follows from the frame's blend_stats counters: a uniform map issues one per MEMBER pair (word 4: every member
        pair has a contribution; word 3, the pairs the forward evaluates, bounds it from above), 64 distinct labels per quadrant
        one per live lane (word 5), two labels between one and two per member pair;
    (b) contrib.lift_mask over the 16-camera orbit, the whole call (16 exact forwards, 16 count read-backs, 16 replays), with a
        disc in the middle of every view as the mask; how many Gaussians it selects, against the Gaussians whose CENTRE projects
        into the disc of some view -- what a selection that does not ask the blend ("all in the frustum and under the mask",
        seen or not) returns -- and against those any view shows at all (peak > 0).

A window is two device events around one call and ends in a synchronise; per form the median, quartiles, extremes and the
medians of the two halves of the windows.  Needs a GPU.

    python tools/votes_time.py [--out profiles/votes.json] [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.contrib_time import H, W, alternate, model  # noqa: E402


def label_maps(dev):
    """name -> (int32 [H*W] on the device, K)"""
    y, x = np.mgrid[0:H, 0:W]
    maps = {"uniform": (np.zeros((H, W), np.int32), 2), "half_plane": ((3 * x + y > 3 * (W // 2) + 5).astype(np.int32), 2),
            "checkerboard": (((x + y) & 1).astype(np.int32), 2), "64_per_quadrant": (((x % 8) + 8 * (y % 8)).astype(np.int32), 64)}
    return {n: (torch.from_numpy(np.ascontiguousarray(m.reshape(-1))).to(dev), K) for n, (m, K) in maps.items()}


def kernel_row(P, dev, reps):
    from goi_hyperplane_amd import _C, contrib
    from goi_hyperplane_amd.render import PipelineParams, render
    pc, cams = model(P, dev)
    cam, bg = cams[0], torch.zeros(3, device=dev)
    S = int(pc.get_semantics.shape[1])
    for _ in range(3):  # (the exact forward that frame_votes drives)
        n, geom, binning, img = contrib._exact_forward(cam, pc, bg, 1.0, None, "votes_time")[3:]
    n = int(n)
    stats = _C.blend_stats(P, W, H, n, geom, binning, img)
    maps = label_maps(dev)
    peak = torch.zeros(P, device=dev)
    out = {name: torch.zeros((P, K), dtype=torch.int64, device=dev) for name, (_, K) in maps.items()}
    forms = {"contrib_peak_from_zero": (peak.zero_, lambda: contrib.frame_buffers(P, W, H, n, geom, binning, img, peak=peak, want_ids=False))}
    for name, (lab, K) in maps.items():
        forms["votes_" + name] = (out[name].zero_, lambda lab=lab, K=K, v=out[name]: contrib.votes_buffers(P, W, H, n, geom, binning, img, lab, K, votes=v))

    def backward_route(lab):
        G = torch.zeros((S, H * W), device=dev)
        G[0], G[1] = (lab == 0).float(), (lab == 1).float()
        G = G.reshape(S, H, W)

        def run():
            pc._semantics.grad = None
            render(cam, pc, PipelineParams(), bg)["semantics"].backward(G)
        return run

    for name in ("uniform", "half_plane", "checkerboard"):
        forms["forward_plus_semantics_backward_" + name] = (lambda: None, backward_route(maps[name][0]))
    res = alternate(forms, reps)
    # what the two routes compute, compared once: the backward's fp32 sums against the exact votes
    backward_route(maps["half_plane"][0])()
    grad = pc._semantics.grad[:, :2].double()
    out["half_plane"].zero_()
    v = contrib.votes_buffers(P, W, H, n, geom, binning, img, maps["half_plane"][0], 2, votes=out["half_plane"])
    again = contrib.votes_buffers(P, W, H, n, geom, binning, img, maps["half_plane"][0], 2)
    assert torch.equal(v, again), "the votes differ between two runs"
    diff = float((v.double() * 2.0 ** -24 - grad).abs().max())
    member, live, fwd_pairs = stats["member_pairs"], stats["live_lanes"], stats["forward_pairs"]
    med = {k: r["median_ms"] for k, r in res.items()}
    row = {"P": P, "W": W, "H": H, "S": S, "num_rendered": n, "windows": res,
           "atomics": {"uniform_exact_member_pairs": member, "uniform_upper_bound_forward_pairs": fwd_pairs,
                       "half_plane_and_checkerboard_between": [member, min(2 * member, live)], "64_per_quadrant_exact_live_lanes": live},
           "ratio_to_contrib_peak": {k[6:]: round(med[k] / med["contrib_peak_from_zero"], 3) for k in med if k.startswith("votes_")},
           "ratio_to_forward_plus_backward": {n_: round(med["votes_" + n_] / med["forward_plus_semantics_backward_" + n_], 3)
                                              for n_ in ("uniform", "half_plane", "checkerboard")},
           "mixed_over_uniform": {n_: round(med["votes_" + n_] / med["votes_uniform"], 3) for n_ in ("half_plane", "checkerboard", "64_per_quadrant")},
           "backward_passes_for_K64": -(-64 // S),
           "half_plane_max_abs_votes_minus_backward_grad": diff, "half_plane_max_grad": float(grad.abs().max()),
           "gaussians_with_a_vote": int((v.sum(1) > 0).sum())}
    pc._semantics.grad = None
    return row, pc, cams


def orbit_row(pc, cams, dev, reps):
    from goi_hyperplane_amd import contrib
    P = int(pc.get_xyz.shape[0])
    bg = torch.zeros(3, device=dev)
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    r = 0.25 * H
    disc = ((x - W / 2) ** 2 + (y - H / 2) ** 2 <= r * r)
    masks = disc[None, None].expand(len(cams), 1, H, W)
    sel = contrib.lift_mask(cams, pc, bg, masks)
    sweep = alternate({"lift_mask_16_cameras": (lambda: None, lambda: contrib.lift_mask(cams, pc, bg, masks))}, max(reps // 3, 6), warmup=1)
    assert torch.equal(contrib.lift_mask(cams[::-1], pc, bg, masks), sel)
    peak = contrib.peak_weights(cams, pc, bg)
    # centres that project into the disc of some view, seen or not
    xyz1 = torch.cat([pc.get_xyz.detach(), torch.ones(P, 1, device=dev)], 1)
    under = torch.zeros(P, dtype=torch.bool, device=dev)
    for c in cams:
        h = xyz1 @ c.full_proj_transform
        wq = h[:, 3]
        px = ((h[:, 0] / wq + 1) * W - 1) * 0.5
        py = ((h[:, 1] / wq + 1) * H - 1) * 0.5
        under |= (wq > 0.2) & ((px - W / 2) ** 2 + (py - H / 2) ** 2 <= r * r)
    return {"P": P, "cameras": len(cams), "mask": f"a disc of radius {r:.0f} pixels in the middle of every view", "sweep": sweep,
            "selected_by_lift_mask": int(sel.sum()), "centre_under_the_mask_of_some_view": int(under.sum()),
            "selected_and_centre_under_the_mask": int((sel & under).sum()), "shown_by_some_view_peak_above_0": int((peak > 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "votes.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/votes_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _C, _lib
    from goi_hyperplane_amd.scene import HEADLINE
    _lib.load()
    doc = {"what": "blend-weight votes per (Gaussian, label) against contrib_k's peak and against forward + semantics backward with a "
                   "one-hot upstream, and one lift_mask over the 16-camera orbit; tools/votes_time.py",
           "device": torch.cuda.get_device_name(dev), "binding": _C.binding(),
           "statistic": "two device events around one call, the window ending in a synchronise; forms alternate in one process after "
                        "warm-up; median, quartiles, extremes, medians of the two halves"}
    doc["kernel"], pc, cams = kernel_row(HEADLINE["P"], dev, args.reps)
    print(json.dumps(doc["kernel"]), flush=True)
    doc["orbit"] = orbit_row(pc, cams, dev, args.reps)
    print(json.dumps(doc["orbit"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
