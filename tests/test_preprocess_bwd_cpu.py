"""The fp32 chain of the per-Gaussian backward (the oracle's goi_oracle_preprocess_backward, plain and FMA-contracted build)
against float64 autograd of the forward of one Gaussian (tests/preprocess_reference.py).  No GPU.

Rounding on this chain is tiny at the median and has a long tail on ill-conditioned rows, so no constant bound is named:
the yardstick is a SECOND, independent fp32 evaluation of the same function, the float32 autograd of the same reference on
the same inputs.  Per tensor and class of Gaussian the oracle's row error max_j|oracle - f64| / max_j|f64| may exceed the
yardstick's by at most 4 x at the median and the 99th percentile and 16 x at the maximum (measured ratios: 0.3 .. 2.5 and 9.6,
docs/MEASUREMENT_LOG.md).  A wrong sign, term or coefficient moves a class's median by five orders of magnitude.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import preprocess_reference as PR

# (tag, P, pose, make_inputs keywords): the camera inside the cloud and its two other poses, the canonical outside camera, every
# SH degree, quaternions of norm 0.5 .. 2, needles (aspect ratio > 100)
RUNS = [
    ("inside", 40000, "inside", {}),
    ("corner", 20000, "corner", {}),
    ("narrow", 20000, "narrow", {}),
    ("outside", 3000, "outside", {}),
    ("deg0", 20000, "inside", dict(sh_degree=0)),
    ("deg1", 20000, "inside", dict(sh_degree=1, M=4)),
    ("deg2", 20000, "inside", dict(sh_degree=2, M=9)),
    ("qnorm", 20000, "inside", dict(qnorm=True, scale_modifier=1.6)),
    ("needles", 20000, "inside", dict(log_scale_std=2.0, scale_modifier=0.7)),
]
EXTRA_CLASS = {"deg0": "deg0", "deg1": "deg1", "deg2": "deg2", "inside": "deg3", "qnorm": "qnorm"}


@pytest.fixture(scope="module")
def pooled(oracle_mod):
    """{evaluation: {(tensor, class): row errors against float64}} pooled over RUNS, and the class sizes."""
    ev = {"f32 autograd": {}, "oracle plain": {}, "oracle fma": {}}
    for tag, P, pose, kw in RUNS:
        inp = PR.make_inputs(P, pose, **kw)
        radii, clamped, cov3D = PR.oracle_forward(oracle_mod, inp)
        k = PR.chain_kwargs(inp)
        mask = PR.clamp_bits(clamped)
        r64 = PR.gaussian_gradients(torch.float64, clamp_mask=mask, **k)
        got = {"f32 autograd": PR.gaussian_gradients(torch.float32, clamp_mask=mask, **k)}
        for name, variant in (("oracle plain", ""), ("oracle fma", "fma")):
            got[name] = oracle_mod.preprocess_backward(radii=radii, clamped=clamped, cov3D=cov3D, variant=variant, **k)
        vis = radii > 0
        cls = PR.classes(r64, vis, inp["scales"])
        if tag in EXTRA_CLASS:
            cls[EXTRA_CLASS[tag]] = vis
        for name, g in got.items():
            for t in PR.TENSORS:
                e = PR.row_error(g[t], r64[t])
                # a row the reference holds as exact zeros (every colour channel clamped): exact zeros in fp32 as well
                dead = vis & np.isnan(e)
                assert not np.any(np.asarray(g[t]).reshape(P, -1)[dead]), f"{name} {t} [{tag}]: non-zero where float64 is zero"
                for c, m in cls.items():
                    ev[name].setdefault((t, c), []).append(e[m])
            if name.startswith("oracle"):  # an invisible Gaussian: zeros in every output
                for t in PR.TENSORS:
                    assert not np.any(np.asarray(g[t]).reshape(P, -1)[~vis]), f"{name} {t} [{tag}]: invisible rows not zero"
    return {n: {k: np.concatenate(v) for k, v in d.items()} for n, d in ev.items()}


def test_every_class_holds_enough_rows(pooled):
    sizes = {k[1]: int((~np.isnan(v)).sum()) for k, v in pooled["oracle plain"].items() if k[0] == "means3D"}
    print(sizes)
    want = {"all", "unclamped", "x_only", "y_only", "both", "near", "deg0", "deg1", "deg2", "deg3", "qnorm", "aspect100"}
    assert want <= set(sizes)
    small = {c: n for c, n in sizes.items() if n < PR.MIN_ROWS}
    assert not small, f"classes below {PR.MIN_ROWS} rows: {small}"


@pytest.mark.parametrize("build", ["oracle plain", "oracle fma"])
def test_oracle_chain_is_as_accurate_as_a_second_fp32_evaluation(pooled, build):
    bad = PR.judge(pooled[build], pooled["f32 autograd"], build)
    assert not bad, "\n".join(bad)


def test_a_wrong_coefficient_is_caught(oracle_mod):
    """The check bites: with the off-diagonal convention wrong (dL_dconic[:, 1] taken as the full gradient) the medians of the
    covariance path move from 1e-7 to 0.1 and more, far outside 4 x the yardstick."""
    inp = PR.make_inputs(20000, "inside")
    radii, clamped, cov3D = PR.oracle_forward(oracle_mod, inp)
    k = PR.chain_kwargs(inp)
    mask = PR.clamp_bits(clamped)
    r64 = PR.gaussian_gradients(torch.float64, clamp_mask=mask, **k)
    r32 = PR.gaussian_gradients(torch.float32, clamp_mask=mask, **k)
    wrong = dict(k)
    wrong["dL_dconic"] = k["dL_dconic"] * np.array([1, 2, 1, 1], np.float32)
    got = oracle_mod.preprocess_backward(radii=radii, clamped=clamped, cov3D=cov3D, **wrong)
    vis = radii > 0
    err = {(t, "all"): PR.row_error(got[t], r64[t])[vis] for t in ("cov3D", "scales", "rotations")}
    yard = {(t, "all"): PR.row_error(r32[t], r64[t])[vis] for t in ("cov3D", "scales", "rotations")}
    bad = PR.judge(err, yard, "wrong b", log=lambda s: None)
    assert len(bad) == 9, bad
    assert all(PR.quantiles(e)[0] > 0.05 for e in err.values())
