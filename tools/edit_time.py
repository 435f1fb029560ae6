"""Times the rigid edit of a selection (goi_hyperplane_amd.edit.transform, csrc/edit.hip) against the same
edit restated in torch on the same device, and writes profiles/edit.json.

    workload   1 M Gaussians, SH degree 3 (M = 16), S = 16, a stepped 7-group Adam state; 10 %, 50 % and 100 % selected at random
    the edit   a 2 degree turn about the selection's centroid, a small translation, and a uniform scale that alternates between
               1.25 and 0.8 from window to window (so the model neither grows nor shrinks over the run): every tensor the edit
               can write is written, the first moments included
    kernel     edit.transform(g, sel, rotation=, translation=, scale=, pivot="centroid"): two launches for the centroid, one for
               parameters and moments, no host synchronisation
    torch      boolean-mask indexing of every tensor, the centroid by mean, (x - p) @ (s R)^T + p + t, the quaternion product
               written out, one matmul per SH band, index-put -- and the same for the three first moments
    viewer     the edit followed by an in-place 1600 x 1056 render of the selection (render(..., gaussian_mask=sel, in_place=True)
               under torch.no_grad()) per frame, both ways

Both paths are warmed and then ALTERNATE in the same process: --reps windows each, a window being two device events around one
edit (one frame) and ending in a synchronise.  Recorded per path: median, quartiles, extremes and the medians of the two halves of
the windows.  A single edit's window holds the host's preparation of the call (the float64 constants, about 0.15 ms of Python)
in front of three short launches, so the kernel path is also timed with 8 edits queued per window: there the host prepares the
next edit while the device runs the last one, and the window over 8 is what one edit costs whichever side is slower.  The
kernel's algorithmic bytes (what it has to read and write for the selected rows: 107 floats in and out, the selection bytes
twice, the positions once more for the centroid) over that time give the achieved bytes per second, stated against the
6.29 TB/s streaming figure of this device.  Needs a GPU.

    python tools/edit_time.py [--out profiles/edit.json] [--reps 30]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

STREAM_TBS = 6.29
FRACTIONS = (0.1, 0.5, 1.0)
QUEUED = 8  # edits per window of the queued figure (an even number: the alternating scales cancel)


def spread(ts):
    q = statistics.quantiles(ts, n=4)
    half = len(ts) // 2
    return {"median_ms": round(statistics.median(ts), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4),
            "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "median_first_half_ms": round(statistics.median(ts[:half]), 4),
            "median_second_half_ms": round(statistics.median(ts[half:]), 4), "windows": len(ts)}


def alternate(paths, reps):
    """paths: {name: callable(window index) running one window's work} -> {name: spread}"""
    times = {n: [] for n in paths}
    for w in range(reps):
        for name, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn(w)
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: spread(ts) for name, ts in times.items()}


def build_model(P, dev):
    """A reference-style model holding the headline scene (raw parameters), with a 7-group Adam stepped twice."""
    from goi_hyperplane_amd.scene import HEADLINE, make_scene
    from tests import densify_reference as dref
    sc = make_scene(P, S=HEADLINE["S"], sh_degree=3, seed=0, extent=HEADLINE["extent"], log_scale_mean=HEADLINE["log_scale_mean"],
                    log_scale_std=HEADLINE["log_scale_std"])
    t = lambda a: torch.nn.Parameter(torch.tensor(a, dtype=torch.float32, device=dev).contiguous())  # noqa: E731
    m = dref.Model()
    m._xyz, m._scaling, m._rotation = t(sc.means3D), t(np.log(sc.scales)), t(sc.rotations)
    m._opacity = t(np.log(sc.opacities / (1 - sc.opacities)))
    m._features_dc, m._features_rest, m._semantics = t(sc.shs[:, :1]), t(sc.shs[:, 1:]), t(sc.semantics)
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, attr)], "lr": 1e-4, "name": name} for name, attr in dref.PARAMS],
                                   lr=0.0, eps=1e-15)
    gen = torch.Generator(device=dev).manual_seed(1)
    for _ in range(2):
        for _, attr in dref.PARAMS:
            p = getattr(m, attr)
            p.grad = 1e-3 * torch.randn(p.shape, device=dev, generator=gen)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    return m


def quat_left(a, b):
    b0, b1, b2, b3 = b.unbind(1)
    return torch.stack([a[0] * b0 - a[1] * b1 - a[2] * b2 - a[3] * b3, a[0] * b1 + a[1] * b0 + a[2] * b3 - a[3] * b2,
                        a[0] * b2 - a[1] * b3 + a[2] * b0 + a[3] * b1, a[0] * b3 + a[1] * b2 - a[2] * b1 + a[3] * b0], dim=1)


class TorchEdit:
    """The edit restated in torch: constants on the device once, then mask indexing, matmuls and index-put per call."""

    def __init__(self, R, t, dev):
        from goi_hyperplane_amd import edit
        f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)  # noqa: E731
        D = edit.sh_rotation(R)
        self.R, self.q, self.t = f(R), f(edit._matrix_to_quat(R)), f(t)
        self.D = [f(D[1:4, 1:4]), f(D[4:9, 4:9]), f(D[9:16, 9:16])]

    def bands(self, f):
        return torch.cat([self.D[0] @ f[:, 0:3], self.D[1] @ f[:, 3:8], self.D[2] @ f[:, 8:15]], dim=1)

    @torch.no_grad()
    def __call__(self, g, sel, s):
        x = g._xyz[sel]
        p = x.mean(dim=0)
        g._xyz[sel] = (x - p) @ (s * self.R).T + p + self.t
        g._rotation[sel] = quat_left(self.q, g._rotation[sel])
        g._scaling[sel] = g._scaling[sel] + math.log(s)
        g._features_rest[sel] = self.bands(g._features_rest[sel])
        st = g.optimizer.state
        m = st[g._xyz]["exp_avg"]
        m[sel] = m[sel] @ self.R.T
        m = st[g._rotation]["exp_avg"]
        m[sel] = quat_left(self.q, m[sel])
        m = st[g._features_rest]["exp_avg"]
        m[sel] = self.bands(m[sel])


def check_paths_agree(dev, R, t):
    """one edit both ways on two small copies of the same model: the same result to fp32 rounding"""
    from goi_hyperplane_amd import edit
    a, b = build_model(20000, dev), build_model(20000, dev)
    sel = torch.rand(20000, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) < 0.5
    edit.transform(a, sel, rotation=R, translation=t, scale=1.25, pivot="centroid")
    TorchEdit(R, t, dev)(b, sel, 1.25)
    worst = 0.0
    for attr in ("_xyz", "_rotation", "_scaling", "_features_rest"):
        worst = max(worst, float((getattr(a, attr).detach() - getattr(b, attr).detach()).abs().max()))
        ma, mb = a.optimizer.state[getattr(a, attr)]["exp_avg"], b.optimizer.state[getattr(b, attr)]["exp_avg"]
        worst = max(worst, float((ma - mb).abs().max()))
    assert worst < 1e-4, worst
    return worst


def algorithmic_bytes(P, n_sel):
    """parameters and first moments of the selected rows in and out (3 + 4 + 3 + 45 + 3 + 4 + 45 floats), the selection bytes for
    the bounds and for the transform, the selected positions once more for the centroid"""
    return n_sel * (107 * 4 * 2 + 12) + 2 * P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--P", type=int, default=1_000_000)
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps must be at least 30")
    assert torch.cuda.is_available(), "tools/edit_time.py needs a GPU"
    dev = torch.device("cuda:0")
    from goi_hyperplane_amd import _C, _lib, edit
    from goi_hyperplane_amd.render import PipelineParams, TorchCamera, render
    from goi_hyperplane_amd.scene import HEADLINE, make_orbit_cameras
    _lib.load()
    ang = math.radians(2.0)
    axis = np.array([0.3, 0.9, 0.2]) / np.linalg.norm([0.3, 0.9, 0.2])
    R = edit._quat_to_matrix(np.concatenate([[math.cos(ang / 2)], math.sin(ang / 2) * axis]))
    t = (0.002, -0.001, 0.0015)
    scale_of = lambda w: 1.25 if w % 2 == 0 else 0.8  # noqa: E731
    agree = check_paths_agree(dev, R, t)
    P = args.P
    g = build_model(P, dev)
    torch_edit = TorchEdit(R, t, dev)
    cam = TorchCamera(make_orbit_cameras(1600, 1056, n=8)[0], dev)
    bg = torch.zeros(3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for frac in FRACTIONS:
        sel = torch.rand(P, device=dev, generator=gen) < frac if frac < 1.0 else torch.ones(P, dtype=torch.bool, device=dev)
        n_sel = int(sel.sum())

        def kernel(w):
            edit.transform(g, sel, rotation=R, translation=t, scale=scale_of(w), pivot="centroid")

        def restated(w):
            torch_edit(g, sel, scale_of(w))

        def show():
            with torch.no_grad():
                render(cam, g, PipelineParams(), bg, gaussian_mask=sel, in_place=True)

        def kernel_frame(w):
            kernel(w)
            show()

        def restated_frame(w):
            restated(w)
            show()

        for w in range(4):  # warm-up of both paths, an even number of windows: the scales cancel
            kernel_frame(w)
            restated_frame(w)
        _C.poll_counts(wait=True)
        edits = alternate({"torch": restated, "kernel": kernel}, args.reps)
        frames = alternate({"torch": restated_frame, "kernel": kernel_frame}, args.reps)
        queued = alternate({"kernel": lambda w: [kernel(2 * w + k) for k in range(QUEUED)]}, args.reps)["kernel"]
        per_edit = queued["median_ms"] / QUEUED
        nbytes = algorithmic_bytes(P, n_sel)
        tbs = nbytes / (per_edit * 1e-3) / 1e12
        row = {"selected_fraction": frac, "selected": n_sel, "edit": edits, "viewer_frame": frames,
               "speedup_edit_median": round(edits["torch"]["median_ms"] / edits["kernel"]["median_ms"], 2),
               "speedup_viewer_frame_median": round(frames["torch"]["median_ms"] / frames["kernel"]["median_ms"], 3),
               "kernel_quartiles_below_torch": bool(edits["kernel"]["q3_ms"] < edits["torch"]["q1_ms"]),
               "kernel_queued": dict(queued, edits_per_window=QUEUED, ms_per_edit=round(per_edit, 4)),
               "kernel_algorithmic_bytes": nbytes, "kernel_tb_per_s": round(tbs, 3),
               "fraction_of_streaming_6p29_tb_per_s": round(tbs / STREAM_TBS, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = {"what": "edit.transform (rigid edit of a selection in place: positions, quaternions, log-scales, SH bands 1..3 and the Adam "
                   "first moments; centroid pivot derived on the device) against the same edit restated in torch; tools/edit_time.py",
           "device": torch.cuda.get_device_name(dev), "P": P, "sh_degree": 3, "S": HEADLINE["S"], "adam_state": "7 groups, stepped twice",
           "edit": "2 degree turn about the selection's centroid, translation (0.002, -0.001, 0.0015), scale alternating 1.25 / 0.8",
           "viewer_frame": "the edit plus an in-place 1600 x 1056 render of the selection under no_grad",
           "paths_agree_max_abs": agree, "streaming_tb_per_s": STREAM_TBS,
           "statistic": "two device events around one edit (one frame), the window ending in a synchronise; the two paths alternate in "
                        "one process after four warm-up rounds of both; median, quartiles, extremes and the medians of the two halves; "
                        "kernel_queued: the same windows around 8 edits in a row, kernel_tb_per_s from its time per edit",
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
