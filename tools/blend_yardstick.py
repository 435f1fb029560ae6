"""The float32 yardstick of the blend-row tolerance (tests/blend_reference.py, docs/MEASUREMENT_LOG.md "Direct test of the blend
kernels"), measured on the CPU: every run of tests/blend_cases.py::all_runs on a frame made from the oracle's records (lists of
the 3-sigma rectangles, float32 direct-form alphas standing in for the device's), the float64 reference against
  * the plain float32 replay of the kernel header's formulation (six moments, expansion)  -- the YARDSTICK, and
  * the float32 replay that forms dx per pixel as the reference's backward.cu does        -- for context.
Prints, per element class, median / p99 / max of |x - f64| / M in units of 2^-24, pooled over the runs.

    python tools/blend_yardstick.py [case ...]
    python tools/blend_yardstick.py --widths     (the 32 frames of tests/channel_count_cases.py, S = 1..32)
    python tools/blend_yardstick.py --all        (both sets, pooled: what tests/blend_reference.py::GATE records)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import blend_cases as BC  # noqa: E402
from tests import blend_reference as BR  # noqa: E402
from tests import channel_count_cases as CC  # noqa: E402


def oracle_frame(sc, cam, bg):
    from oracle import oracle
    oracle.build()
    o = oracle.from_scene(sc, cam, bg=bg)
    f = o.forward()
    st = o.state()
    W, H = cam.image_width, cam.image_height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    px, py, r = st["means2D"][:, 0].astype(np.float32), st["means2D"][:, 1].astype(np.float32), f.radii.astype(np.float32)
    t = lambda v, g: np.minimum(g, np.maximum(0, (v / np.float32(16)).astype(np.int64)))  # noqa: E731
    rects = np.stack([t(px - r, gx), t(py - r, gy), t(px + r + 15, gx), t(py + r + 15, gy)], 1)
    rects[f.radii <= 0] = 0
    return BR.cpu_frame(W, H, st["means2D"], st["conic_opacity"], st["rgb"], st["depths"], sc.semantics, bg, rects=rects)


def main(names):
    # --widths: the 32 frames of tests/channel_count_cases.py instead of blend_cases.all_runs(); --all: both, pooled
    width_runs = [(f"width{S}", S) for S in CC.WIDTHS]
    if names in (["--widths"], ["--all"]):
        runs = width_runs + (BC.all_runs() if names == ["--all"] else [])
    else:
        runs = [r for r in BC.all_runs() if not names or r[0] in names]
    S_list, y_err, d_err = [], [], []
    for name, kind in runs:
        if isinstance(kind, int):
            sc, cam = CC.case(kind)
            up, bg, kind = CC.upstream_dict(kind), CC.BG, "random"
        else:
            sc, cam = BC.ROW_CASES[name]()
            up, bg = BC.upstream(kind, sc.S, cam.image_height, cam.image_width, name)
        fr, qd, E, alpha, hit = oracle_frame(sc, cam, bg)
        ref = BR.backward_rows(fr, qd, up, E, alpha, hit)
        if not ref.member.any():
            print(f"{name}/{kind}: no member pair")
            continue
        y = BR.backward_rows(fr, qd, up, E, alpha, hit, dtype=np.float32)
        d = BR.backward_rows(fr, qd, up, E, alpha, hit, dtype=np.float32, direct_moments=True)
        ey, _ = BR.normalised_errors(sc.S, ref, y.rows)
        ed, _ = BR.normalised_errors(sc.S, ref, d.rows)
        S_list.append(sc.S)
        y_err.append(ey)
        d_err.append(ed)
        st = BR.class_stats(sc.S, ey)
        print(f"{name}/{kind}: {int(ref.member.sum())} rows, depth <= {int(ref.depth.max())}; yardstick max "
              + " ".join(f"{c}={st[c][2] / BR.U:.2f}" for c in BR.CLASSES), flush=True)
    for title, errs in (("yardstick (moments + expansion)", y_err), ("direct dx per pixel (backward.cu order)", d_err)):
        print(f"\n{title}: median / p99 / max of |x - f64| / M, units of 2^-24, pooled over {len(errs)} runs")
        for c, (med, p99, mx, n) in BR.pooled_stats(S_list, errs).items():
            print(f"  {c:13s} {med / BR.U:8.3f} {p99 / BR.U:8.3f} {mx / BR.U:8.3f}   n = {n}")
    print("\nGATE = {")
    for c, (med, p99, mx, n) in BR.pooled_stats(S_list, y_err).items():
        print(f'    "{c}": ({med / BR.U:.3f} * U, {p99 / BR.U:.3f} * U, {mx / BR.U:.3f} * U),')
    print("}")


if __name__ == "__main__":
    main(sys.argv[1:])
