#!/usr/bin/env python3
"""Generates tests/golden/ref_osh_pins.npz: the reference's hyperplane fine-tune (gui/main.py:1673-1763,
finetune_prompt_with_res) run on CPU fp32 on seeded inputs.  Run in the AUTHORING container only (it reads the
reference's sources); the fixture is data only.

    python tests/golden/make_osh_golden.py

Nothing of the reference is re-typed: LinearSVM, inverse_sigmoid and hinge_loss (networks.py) and calculate_iou
(utils/image_utils.py) are the reference's own AST nodes (the modules cannot be imported: they pull in cv2); the
normalisation is the method's own `normed_feature = ...` statement and the fit is its own statements from
`epoch = 0` through the `while` loop, executed with a stand-in `self` that carries resMLP, H and W.  The loop
body's PIL / print side effects are stubbed; each LinearSVM.step call is recorded for the per-epoch (loss, IoU) trace.

Each case is checked to be well-conditioned: the float64 per-code restatement (tests/osh_reference.py) must give the
same epoch count and the same IoU trace up to a few isolated epochs (stored as f64_flips); the smallest distance of any
margin to the kinks {-1, 0, 1} (and to 0) is stored.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import _cuda_is_cpu, _exec_stmts, _method, _ref_ast  # noqa: E402
from tests.osh_reference import counts_of, fit_per_code  # noqa: E402


def _ref_namespace():
    net = _ref_ast("networks.py")
    ns = {"torch": torch, "nn": torch.nn, "optim": torch.optim, "F": torch.nn.functional}
    util = _ref_ast("utils/image_utils.py")
    _exec_stmts([n for n in util.body if isinstance(n, ast.FunctionDef) and n.name == "calculate_iou"], ns,
                "utils/image_utils.py")
    _exec_stmts([n for n in net.body if isinstance(n, ast.FunctionDef) and n.name in ("inverse_sigmoid", "hinge_loss")]
                + [n for n in net.body if isinstance(n, ast.ClassDef) and n.name == "LinearSVM"], ns, "networks.py")
    return ns


def _finetune_stmts():
    fn = _method(_ref_ast("gui/main.py"), "GUI", "finetune_prompt_with_res")
    body = fn.body
    norm = next(n for n in ast.walk(fn) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "normed_feature"
                and "norm(" in ast.unparse(n))
    first = next(i for i, n in enumerate(body) if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "epoch")
    last = next(i for i, n in enumerate(body) if isinstance(n, ast.While))
    stmts = body[first:last + 1]
    return norm, stmts, (stmts[0].lineno, stmts[-1].end_lineno)


def run_reference(ns, lut, idx, gt, w0, set_bias, H, W):
    """The reference's statements on CPU fp32; returns (svm, init_iou, trace [epochs, 2], epochs)."""
    norm, stmts, lines = _finetune_stmts()
    svm = ns["LinearSVM"](set_bias=set_bias, input_dim=lut.shape[1])
    svm.weight_set(torch.tensor(w0).reshape(1, -1))
    b0 = svm.linear.bias.detach().clone()
    trace = []
    step = svm.step

    def recorded_step(x, y):
        loss, iou = step(x, y)
        trace.append((loss.item(), iou))
        return loss, iou
    svm.step = recorded_step
    printed = []
    env = {"torch": torch, "sem_feature": torch.tensor(lut)[torch.tensor(idx).long()],
           "self": types.SimpleNamespace(resMLP=svm, H=H, W=W), "gt": torch.tensor(gt).float().reshape(-1, 1),
           "Image": types.SimpleNamespace(fromarray=lambda a: a), "print": lambda *a, **k: printed.append(a)}
    _exec_stmts([norm], env, "gui/main.py:normed_feature")
    env["normed_feature"] = env["normed_feature"].detach()
    with _cuda_is_cpu():
        # the init-IoU print of the method (eval_forward on the initial hyperplane), then its loop
        init_iou = svm.eval_forward(env["normed_feature"], env["gt"])
        _exec_stmts(stmts, env, f"gui/main.py:{lines[0]}-{lines[1]}")
    assert env["epoch"] == len(trace)
    return svm, b0, init_iou, np.array(trace, np.float64), lines


def make_case(rng, n_codes, D, H, W, pos_codes_frac, p_in, p_out, alpha, t, empty=False):
    """Codes are positive (mask mostly 1) or negative; their LUT rows lean by alpha along a direction u, and the
    initial hyperplane (the GUI's text feature) is a unit vector part-aligned with u (weight t)."""
    u = rng.normal(size=D)
    u /= np.linalg.norm(u)
    pos_code = rng.random(n_codes) < pos_codes_frac
    lut = (rng.normal(size=(n_codes, D)) * (1.6 / np.sqrt(D)) + alpha * (2 * pos_code - 1)[:, None] * u[None]).astype(np.float32)
    idx = rng.integers(0, n_codes, size=H * W).astype(np.int32)
    gt = np.where(pos_code[idx], rng.random(H * W) < p_in, rng.random(H * W) < p_out)
    if empty:
        gt[:] = False
    r = rng.normal(size=D)
    r /= np.linalg.norm(r)
    w0 = t * u + (1 - t) * r
    return lut, idx, gt.astype(np.uint8), (w0 / np.linalg.norm(w0)).astype(np.float32)


CASES = {
    # name: (seed, n_codes, D, H, W, pos_codes_frac, p_in, p_out, alpha, t, empty, set_bias)
    "a": (136, 300, 256, 64, 64, 0.3, 0.98, 0.01, 0.2, 0.3, False, 0.86),   # stops on IoU >= 0.9
    "b": (100, 300, 256, 64, 64, 0.3, 0.8, 0.05, 0.2, 0.3, False, 0.86),    # runs all 8000 epochs (IoU capped by label noise)
    "c": (13, 300, 256, 64, 64, 0.3, 0.98, 0.01, 0.2, 0.3, True, 0.999),   # empty mask, nothing predicted: NaN after the first step
    "d": (100, 37, 100, 64, 64, 0.4, 0.97, 0.02, 0.2, 0.3, False, 0.5),     # small odd shape
}


def main():
    ns = _ref_namespace()
    out = {}
    for name, (seed, n_codes, D, H, W, frac, p_in, p_out, alpha, t, empty, set_bias) in CASES.items():
        rng = np.random.default_rng(seed)
        lut, idx, gt, w0 = make_case(rng, n_codes, D, H, W, frac, p_in, p_out, alpha, t, empty)
        svm, b0, init_iou, trace, lines = run_reference(ns, lut, idx, gt, w0, set_bias, H, W)
        w = svm.linear.weight.detach().numpy().reshape(-1)
        b = float(svm.linear.bias.detach())
        chk = fit_per_code(lut, counts_of(idx, gt, n_codes), H * W, w0, float(b0), max_epochs=8000, target_iou=0.9)
        n = min(len(trace), chk["epochs"])
        flips = int((~((chk["trace"][:n, 1] == trace[:n, 1]) | (np.isnan(chk["trace"][:n, 1]) & np.isnan(trace[:n, 1])))).sum())
        print(f"case {name}: epochs {len(trace)} (f64 {chk['epochs']}), init_iou {init_iou:.6f}, final iou {trace[-1, 1]:.6f}, "
              f"kink {chk['kink']:.3g} (to 0: {chk['kink0']:.3g}), |w - w64| {np.abs(w - chk['w']).max():.3g} (max|w| {np.abs(w).max():.3g})")
        # well-conditioned: the same epoch count and the same IoU at all but a few isolated epochs (a margin oscillating
        # within ~1e-5 of 0 after hundreds of steps decides an epoch's IoU at the precision of the arithmetic)
        print(f"  IoU trace vs float64: {flips} epoch(s) differ")
        assert chk["epochs"] == len(trace) and flips <= max(2, len(trace) // 200), f"case {name} is not well-conditioned"
        assert (init_iou == chk["init_iou"]) or (np.isnan(init_iou) and np.isnan(chk["init_iou"]))
        for k, v in dict(lut=lut, idx=idx.astype(np.int16), gt=gt.astype(bool), w0=w0, b0=b0.numpy().reshape(()),
                         trace=trace, w=w, b=np.float32(b), epochs=np.int32(len(trace)), init_iou=np.float64(init_iou),
                         kink=np.float64(chk["kink"]), kink0=np.float64(chk["kink0"]), f64_flips=np.int32(flips), set_bias=np.float32(set_bias),
                         hw=np.array([H, W], np.int32)).items():
            out[f"{name}_{k}"] = v
    out["ref_lines"] = np.array(lines)
    path = os.path.join(HERE, "ref_osh_pins.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; gui/main.py lines", lines)


if __name__ == "__main__":
    main()
