"""Times the non-rigid edit of a selection (goi_hyperplane_amd.deform, csrc/deform.hip) and writes
profiles/deform.json.

    workload   the bench's 1 M Gaussians, SH degree 3 (M = 16), S = 16, a stepped 7-group Adam state; 10 %, 50 % and 100 % selected
               at random; about 4000 control nodes (the spacing is searched for), k = 8, kb = 4
    motion     the nodes with x above the selection's median pinned to a 20 degree turn about z, the lowest tenth pinned in place
    timed      apply (one launch), single and with 8 queued; one solve iteration and 50; the session's construction (sample_nodes,
               graph, transpose, binding) once; commit of a deformed state (the moment turn and the rebuild; the drag, solve and
               apply before each window are not timed); the energy of the naive edit against the solved one is recorded
    against    (a) the same apply restated in torch on the same device: gather the nodes, weights, rotation matrices from
               quaternions, bmm, a per-row SH matrix per band; (b) edit.transform of the same selection in the same windows: the
               rigid lower bound -- the same bytes written, no gathers

Paths alternate in one process after warm-up; a window is two device events around the work and ends in a synchronise; medians
with quartiles (tools/edit_time.py's statistic).  apply's compulsory traffic -- rest rows read (3 + 4 + 45 floats), binding rows
(kb ids and distances), rows written, the selection byte -- is stated against the 6.29 TB/s streaming figure.  Also timed: the
worst case for gather locality, every Gaussian bound to ONE node.  Needs a GPU.

    python tools/deform_time.py [--out profiles/deform.json] [--reps 30]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from edit_time import STREAM_TBS, alternate, build_model, spread  # noqa: E402

FRACTIONS = (0.1, 0.5, 1.0)
QUEUED = 8
TARGET_NODES = 4000


def quat_matrix(q, minus_identity=False):
    w, x, y, z = q.unbind(1)
    one = 0.0 if minus_identity else 1.0
    return torch.stack([one - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z),
                        one - 2 * (x * x + z * z), 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x),
                        one - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def quat_left(a, b):
    a0, a1, a2, a3 = a.unbind(1)
    b0, b1, b2, b3 = b.unbind(1)
    return torch.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3, a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                        a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1, a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0], dim=1)


class TorchApply:
    """deform's apply restated in torch: boolean-mask indexing, gathers, bmm and one [n, 2l+1, 2l+1] SH matrix per band"""

    def __init__(self, dev):
        from goi_hyperplane_amd import deform
        from goi_hyperplane_amd.render import SH_C1, SH_C2, SH_C3
        f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)  # noqa: E731
        self.sh = [(f(d), f(inv)) for d, inv in deform.sh_constants()]
        self.c1, self.c2, self.c3 = SH_C1, SH_C2, SH_C3

    def band(self, u, l):
        x, y, z = u.unbind(-1)
        if l == 1:
            return torch.stack([-self.c1 * y, self.c1 * z, -self.c1 * x], dim=-1)
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        if l == 2:
            c = self.c2
            return torch.stack([c[0] * xy, c[1] * yz, c[2] * (2 * zz - xx - yy), c[3] * xz, c[4] * (xx - yy)], dim=-1)
        c = self.c3
        return torch.stack([c[0] * y * (3 * xx - yy), c[1] * xy * z, c[2] * y * (4 * zz - xx - yy), c[3] * z * (2 * zz - 3 * xx - 3 * yy),
                            c[4] * x * (4 * zz - xx - yy), c[5] * z * (xx - yy), c[6] * x * (xx - 3 * yy)], dim=-1)

    @torch.no_grad()
    def __call__(self, g, rest, sel, bind, nodes, sigma):
        nx, ny, nq = nodes
        idx, d2 = bind[0][sel].long(), bind[1][sel]
        w = torch.exp(-(d2 - d2[:, :1]) / (2 * sigma * sigma))
        w = w / w.sum(dim=1, keepdim=True)
        x = rest[0][sel]
        qa = nq[idx]                                                           # [n, kb, 4]
        Ra = quat_matrix(qa.view(-1, 4), True).view(idx.shape[0], idx.shape[1], 3, 3)
        term = (ny[idx] - nx[idx]) + torch.einsum("nkij,nkj->nki", Ra, x[:, None, :] - nx[idx])
        g._xyz[sel] = x + (w[..., None] * term).sum(dim=1)
        s = torch.where((qa * qa[:, :1]).sum(dim=-1) < 0, -1.0, 1.0)
        qg = torch.nn.functional.normalize(((w * s)[..., None] * qa).sum(dim=1), dim=1)
        g._rotation[sel] = quat_left(qg, rest[1][sel])
        Rg = quat_matrix(qg)
        c = rest[2][sel]
        out = []
        for l, (dirs, inv) in enumerate(self.sh, start=1):
            u = torch.einsum("nji,kj->nki", Rg, dirs)                          # R^T d_k
            D = inv @ self.band(u, l)                                          # [n, 2l+1, 2l+1]
            out.append(torch.bmm(D, c[:, l * l - 1:(l + 1) * (l + 1) - 1]))
        g._features_rest[sel] = torch.cat(out, dim=1)


def spacing_for(xyz, sel, target):
    """a spacing that gives about `target` nodes: bisection on sample_nodes (set-up, not timed)"""
    from goi_hyperplane_amd import deform
    lo, hi = 1e-3, 100.0
    for _ in range(24):
        mid = math.sqrt(lo * hi)
        n = int(deform.sample_nodes(xyz, sel, mid).shape[0])
        if 0.9 * target <= n <= 1.1 * target:
            return mid
        lo, hi = (mid, hi) if n > target else (lo, mid)
    return mid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--P", type=int, default=1_000_000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/deform_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _lib, deform, edit
    from goi_hyperplane_amd.scene import HEADLINE
    _lib.load()
    P = args.P
    g = build_model(P, dev)
    torch_apply = TorchApply(dev)
    half = math.radians(10.0)
    turn = (math.cos(half), 0.0, 0.0, math.sin(half))
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for frac in FRACTIONS:
        sel = torch.rand(P, device=dev, generator=gen) < frac if frac < 1.0 else torch.ones(P, dtype=torch.bool, device=dev)
        n_sel = int(sel.sum())
        spacing = spacing_for(g._xyz.detach(), sel, TARGET_NODES)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = deform.Deformation(g, sel, spacing=spacing, k=8, kb=4)
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        xs = d.x[:, 0]
        d.constrain(xs <= torch.quantile(xs, 0.1), d.x[xs <= torch.quantile(xs, 0.1)])
        d.drag(xs >= torch.quantile(xs, 0.5), rotation=turn)
        # convergence: the naive edit (only the pinned and dragged nodes moved, no rotation) against the solve
        ident = torch.zeros_like(d.q)
        ident[:, 0] = 1.0
        E_naive = float(deform.energy(d.x, d.idx, torch.where(d.constrained.bool().unsqueeze(1), d.target, d.x), ident))
        E_50 = float(d.solve(iterations=50).energy())
        solve = alternate({"one_iteration": lambda w: d.solve(iterations=1), "fifty_iterations": lambda w: d.solve(iterations=50)}, args.reps)
        n_iter = 50 + 51 * args.reps
        E_end = float(d.energy())
        nodes = (d.x, d.y, d.q)

        def kernel(w):
            d.apply()

        def restated(w):
            torch_apply(g, d.rest, sel, d.bind, nodes, d.sigma)

        def rigid(w):  # the rigid lower bound, there and back so that the model does not drift
            edit.transform(g, sel, rotation=turn if w % 2 == 0 else (turn[0], 0.0, 0.0, -turn[3]), pivot="origin", moments=False)

        for w in range(4):
            restated(w), rigid(w), kernel(w)
        agree = 0.0
        restated(0)
        got = [getattr(g, a).detach().clone() for a in ("_xyz", "_rotation", "_features_rest")]
        kernel(0)
        for a, b in zip(got, (g._xyz, g._rotation, g._features_rest)):
            agree = max(agree, float((a - b.detach()).abs().max()))
        assert agree < 1e-4, agree
        applies = alternate({"torch": restated, "edit_transform": rigid, "kernel": kernel}, args.reps)
        queued = alternate({"kernel": lambda w: [kernel(w) for _ in range(QUEUED)]}, args.reps)["kernel"]
        per = queued["median_ms"] / QUEUED
        nbytes = n_sel * ((52 * 2) * 4 + d.kb * 8) + P
        # the worst case for the gathers: every Gaussian bound to one node (and every lane of a wave reads the same node)
        one = (torch.zeros_like(d.bind[0]), torch.zeros_like(d.bind[1]))
        saved, d.bind = d.bind, one
        hub = alternate({"kernel": kernel}, args.reps)["kernel"]
        d.bind = saved
        kernel(0)
        # commit of a DEFORMED state: before every window the handle is dragged a little further, solved and applied, untimed
        handle = torch.nonzero(d.constrained.bool() & ((d.target - d.x).abs().sum(dim=1) > 0)).squeeze(1)
        ts = []
        for w in range(max(args.reps // 3, 10) + 2):
            d.drag(handle, rotation=turn if w % 2 == 0 else (turn[0], 0.0, 0.0, -turn[3])).solve(iterations=10).apply()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            d.commit()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        commit = spread(ts[2:])  # (two warm-up windows)
        d.reset()
        row = {"selected_fraction": frac, "selected": n_sel, "nodes": d.M, "spacing": round(spacing, 5), "k": d.k, "kb": d.kb,
               "session_build_ms_once": round(build_ms, 3), "solve": solve,
               "energy": {"naive_edit": E_naive, "after_50_iterations": E_50, "after_all_timed_iterations": E_end, "iterations_in_all": n_iter},
               "apply": applies, "apply_queued": dict(queued, per_window=QUEUED, ms_per_apply=round(per, 4)),
               "apply_every_gaussian_bound_to_one_node": hub, "commit": commit, "paths_agree_max_abs": agree,
               "torch_over_apply": round(applies["torch"]["median_ms"] / applies["kernel"]["median_ms"], 2),
               "apply_over_edit_transform": round(applies["kernel"]["median_ms"] / applies["edit_transform"]["median_ms"], 2),
               "apply_compulsory_bytes": nbytes, "apply_tb_per_s": round(nbytes / (per * 1e-3) / 1e12, 3),
               "fraction_of_streaming_6p29_tb_per_s": round(nbytes / (per * 1e-3) / 1e12 / STREAM_TBS, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = {"what": "deform (as-rigid-as-possible deformation of a selection: solve on the node graph, apply to the Gaussians with SH bands "
                   "1..3 rotated per row, commit with the Adam first moments) against the apply restated in torch and against the rigid "
                   "edit.transform of the same selection; tools/deform_time.py",
           "device": torch.cuda.get_device_name(dev), "P": P, "sh_degree": 3, "S": HEADLINE["S"], "streaming_tb_per_s": STREAM_TBS,
           "statistic": "two device events around the work, the window ending in a synchronise; the paths alternate in one process after "
                        "warm-up; median, quartiles, extremes and the medians of the two halves; call-level times (host preparation "
                        "included), kernel times were not taken",
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
