"""What the direct tests of the fused Adam step (tests/test_gpu_adam_direct.py) rest on, checked without a GPU.

The gate there is bit for bit against oracle.adam_step.  Here:

* the gate is SENSITIVE: on the GPU tests' own input distribution (adam_reference.normal_inputs, P = 4099) each of the
  mis-spellings a compiler or a hand could introduce differs from the oracle in the tensor it touches.  Measured shares
  of the 4099 elements (printed by the test): exp_avg as one FMA 20.91 % (857), exp_avg_sq as one FMA 3.03 % (124),
  exp_avg_sq re-associated as beta2 v + (1 - beta2)(g g) 1.90 % (78), param as one FMA 0.78 % (32).
* the oracle is ACCURATE: over 50 steps at P = 1021 on the reference's seven groups, its distance from a float64 run
  of the same update is held to 2 x the distance of torch.optim.Adam (fp32, CPU) from that run, plus one fp32 ulp of the
  tensor's largest magnitude.  Measured (printed by the test), max over steps, elements and the seven groups:
      tensor        oracle - float64   torch - float64   ratio   worst ratio of one group
      param         2.088e-06          2.088e-06         1.00    1.00
      exp_avg       7.865e-08          7.207e-08         1.09    1.17
      exp_avg_sq    2.468e-08          2.799e-08         0.88    1.00
* the two per-step SCALARS optim.py hands the kernel are the oracle's and torch's (`** 0.5`, not math.sqrt: in double the
  two differ at 6 of t = 1..5000 at beta2 = 0.999), fp32-rounded, for t = 1..5000 and every beta pair the tests use;
* the denormal, zero, -0.0, inf, NaN and overflow tables of the GPU test go through the oracle and the float64 form first.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import adam_reference as ar
from tests.test_adam_cpu import GROUPS, LRS, make_params, reference_groups

F = np.float32
BETAS = [(0.9, 0.999), (0.0, 0.999), (0.9, 0.0), (0.5, 0.9)]
EPSS = [1e-8, 1e-15, 0.0]
STEPS = [1, 2, 10, 1000, 30000]


def f32(x):
    return ctypes.c_float(x).value


def test_spelled_form_is_the_oracle():
    """adam_spelled (explicit scalars, replaceable lines) with no variant IS oracle.adam_step, at every hyper-parameter
    the tests use: what the variants below are measured against is the oracle itself."""
    p, g, m, v = ar.normal_inputs(4099, 0)
    for beta1, beta2 in BETAS:
        for eps in EPSS:
            for t in STEPS:
                ss, bc = ar.scalars(1e-2, beta1, beta2, t)
                a = ar.adam_spelled(p, g, m, v, ss, bc, beta1, beta2, eps)
                with np.errstate(all="ignore"):
                    b = oracle.adam_step(p, g, m, v, t, 1e-2, beta1=beta1, beta2=beta2, eps=eps)
                for x, y in zip(a, b):
                    ar.assert_bits(x, y, (beta1, beta2, eps, t))


@pytest.mark.parametrize("variant", sorted(ar.VARIANTS))
def test_gate_is_sensitive(variant):
    p, g, m, v = ar.normal_inputs(4099, 0)
    ss, bc = ar.scalars(1e-2, 0.9, 0.999, 3)
    base = ar.adam_spelled(p, g, m, v, ss, bc, eps=1e-15)
    mut = ar.adam_spelled(p, g, m, v, ss, bc, eps=1e-15, variant=variant)
    i = ar.VARIANTS[variant]
    differ = int(np.count_nonzero(ar.bits(base[i]) != ar.bits(mut[i])))
    print(f"{variant}: {differ} of {p.size} elements differ ({100.0 * differ / p.size:.2f} %)")
    assert differ >= 1


def test_oracle_stays_inside_the_float64_yardstick():
    P, steps = 1021, 50
    params = make_params(P)
    opt = torch.optim.Adam(reference_groups(params), lr=0.0, eps=1e-15)
    mine = {k: (v.detach().numpy().copy(), np.zeros(v.shape, F), np.zeros(v.shape, F)) for k, v in params.items()}
    ref = {k: (v.detach().numpy().astype(np.float64), np.zeros(v.shape), np.zeros(v.shape)) for k, v in params.items()}
    err_o = {(k, i): 0.0 for k in GROUPS for i in range(3)}
    err_t = dict(err_o)
    mag = dict(err_o)
    rng = np.random.default_rng(0)
    for step in range(1, steps + 1):
        for k, v in params.items():
            gr = (rng.standard_normal(v.shape) * (10.0 ** rng.integers(-6, 1))).astype(F)
            v.grad = torch.from_numpy(gr.copy())
            mine[k] = oracle.adam_step(*mine[k][:1], gr, *mine[k][1:], step, LRS[k], eps=1e-15)
            ref[k] = ar.adam_step64(ref[k][0], gr, ref[k][1], ref[k][2], step, LRS[k], eps=1e-15)
        opt.step()
        for k, v in params.items():
            st = opt.state[v]
            th = (v.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())
            for i in range(3):
                err_o[k, i] = max(err_o[k, i], float(np.abs(mine[k][i] - ref[k][i]).max()))
                err_t[k, i] = max(err_t[k, i], float(np.abs(th[i] - ref[k][i]).max()))
                mag[k, i] = max(mag[k, i], float(np.abs(ref[k][i]).max()))
    names = ("param", "exp_avg", "exp_avg_sq")
    bad = []
    for i in range(3):
        eo = max(err_o[k, i] for k in GROUPS)
        et = max(err_t[k, i] for k in GROUPS)
        worst = max(err_o[k, i] / err_t[k, i] for k in GROUPS)
        print(f"{names[i]}: oracle {eo:.3e}, torch {et:.3e}, ratio of the maxima {eo / et:.2f}, worst group ratio {worst:.2f}")
    for (k, i), eo in err_o.items():
        bound = 2.0 * err_t[k, i] + float(np.spacing(F(mag[k, i])))
        if not eo <= bound:
            bad.append((k, names[i], eo, err_t[k, i], bound))
    assert not bad, bad


def test_float64_form_agrees_with_the_oracle_to_rounding():
    """One step from the same fp32 state: the oracle is within a few fp32 roundings of the float64 form (so adam_step64
    is the same update, not merely a similar one)."""
    p, g, m, v = ar.normal_inputs(4099, 1)
    for beta1, beta2 in BETAS:
        for t in STEPS:
            a = oracle.adam_step(p, g, m, v, t, 1e-2, beta1=beta1, beta2=beta2, eps=1e-8)
            b = ar.adam_step64(p, g, m, v, t, 1e-2, beta1=beta1, beta2=beta2, eps=1e-8)
            # u = 2^-24 per rounding.  m, v: three roundings of operands no larger than max(|g|, |m|) resp. max(v, g^2).
            # p: the error of m over den, the relative error of den (half that of v, two roundings, eps) and of the
            # scalar, quotient and product on the update, one rounding of the sum.
            u = 6e-8
            dm = 3 * u * np.maximum(np.abs(g), np.abs(m))
            dv = 3 * u * np.maximum(v, g.astype(np.float64) ** 2)
            assert np.all(np.abs(a[1] - b[1]) <= dm)
            assert np.all(np.abs(a[2] - b[2]) <= dv)
            ss, bc = ar.scalars(1e-2, beta1, beta2, t)
            den = np.sqrt(b[2]) / bc + 1e-8
            upd = np.abs(b[0] - p)
            tol = u * (np.abs(p) + upd) + ss * dm / den + upd * (0.5 * dv / b[2] + 6 * u)
            assert np.all(np.abs(a[0] - b[0]) <= tol)


def test_scalars_are_torchs_and_the_oracles():
    """optim.bias_scalars against torch/optim/adam.py's spelling (_single_tensor_adam / _multi_tensor_adam, non-capturable:
    `lr / (1 - beta1**step)`, `(1 - beta2**step) ** 0.5`), fp32-rounded as the C struct and the oracle's f() round them."""
    from goi_hyperplane_amd.optim import bias_scalars
    sqrt_differs = 0
    for beta1, beta2 in BETAS:
        for t in range(1, 5001):
            ss, bc = bias_scalars(1e-2, beta1, beta2, float(t))
            bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
            assert f32(ss) == f32(1e-2 / bc1) and ss == 1e-2 / bc1, (beta1, t)
            assert f32(bc) == f32(bc2 ** 0.5) and bc == bc2 ** 0.5, (beta2, t)
            sqrt_differs += (beta2 == 0.999) and (math.sqrt(bc2) != bc2 ** 0.5)
    print("t in 1..5000 at which math.sqrt and ** 0.5 differ in double (beta2 = 0.999):", sqrt_differs)


def test_scalars_reach_the_oracles_bits_at_every_step():
    """The same through the oracle's own code: a 64-element update with optim.py's scalars equals oracle.adam_step bit for
    bit at every t in 1..5000 (the oracle forms its scalars inline; this is how they are compared)."""
    p, g, m, v = ar.normal_inputs(64, 2)
    for beta1, beta2 in BETAS:
        for t in range(1, 5001):
            ss, bc = ar.scalars(LRS["xyz"], beta1, beta2, t)
            a = ar.adam_spelled(p, g, m, v, ss, bc, beta1, beta2, 1e-15)
            b = oracle.adam_step(p, g, m, v, t, LRS["xyz"], beta1=beta1, beta2=beta2, eps=1e-15)
            assert all(np.array_equal(ar.bits(x), ar.bits(y)) for x, y in zip(a, b)), (beta1, beta2, t)


def test_mask_bytes_non_zero_means_masked_in_every_dtype():
    """optim.mask_bytes, the host half of FusedAdam.step(nograd_mask=...): a cast alone wraps 256 to 0 and truncates 0.5."""
    from goi_hyperplane_amd.optim import mask_bytes
    want = np.array([0, 1, 1, 0, 1, 1], bool)
    cases = [torch.tensor([0, 1, 256, 0, -1, 1 << 40], dtype=torch.int64), torch.tensor([0, 1, 65536, 0, -256, 512], dtype=torch.int32),
             torch.tensor([0, 256, 512, 0, 1, -256], dtype=torch.int16), torch.tensor([0.0, 0.5, -1e-30, -0.0, float("nan"), 1e30]),
             torch.tensor([0.0, 0.25, 256.0, 0.0, 1e-300, -0.5], dtype=torch.float64), torch.tensor([0, 1, 1, 0, 1, 1], dtype=torch.bool),
             torch.tensor([0, 1, 2, 0, 0x80, 0xFF], dtype=torch.uint8)]
    for m in cases:
        out = mask_bytes(m, torch.device("cpu"))
        assert out.dtype == torch.uint8 and out.is_contiguous() and np.array_equal(out.numpy() != 0, want), m.dtype
    strided = torch.tensor([0, 9, 256, 9, 256, 9], dtype=torch.int64)[::2]
    assert mask_bytes(strided, torch.device("cpu")).tolist() == [0, 1, 1]


# ---------------------------------------------------------------------------------------------------------------------
# value classes: what the GPU test will expect, pinned here first

VALUE_TABLES = ar.value_class_tables()


@pytest.mark.parametrize("name", sorted(VALUE_TABLES))
def test_value_class_nan_is_where_float64_has_it(name):
    groups, hp = VALUE_TABLES[name]
    want = ar.expect_table(groups, hp["beta1"], hp["beta2"], hp["eps"])
    for gr, (p, m, v) in zip(groups, want):
        p64, m64, v64 = ar.adam_step64(gr["p"], gr["g"], gr["m"], gr["v"], gr["t"], gr["lr"], **hp)
        for a, b in ((p, p64), (m, m64), (v, v64)):
            assert np.array_equal(np.isnan(a), np.isnan(b)), name
        # and where everything is finite in fp32 the two agree to fp32 rounding of the operands
        fin = np.isfinite(p) & np.isfinite(m) & np.isfinite(v) & np.isfinite(gr["g"])
        assert np.all(np.abs(m[fin] - m64[fin]) <= 2e-7 * np.maximum(np.abs(gr["g"]), np.abs(gr["m"]))[fin] + 1.5e-45)


def test_value_class_pins():
    T = VALUE_TABLES
    tiny = np.finfo(F).tiny

    def is_denormal(a):
        return (a != 0) & (np.abs(a) < tiny)

    # zero gradient: denormal moments stay denormal (nothing is flushed), m decays by exactly the fp32 spelling
    groups, hp = T["zero_grad_seeded_moments"]
    for gr, (p, m, v) in zip(groups, ar.expect_table(groups, **hp)):
        dm = is_denormal(gr["m"])
        assert dm.sum() >= 10 and np.all(is_denormal(m[dm]))
        dv = is_denormal(gr["v"])
        assert np.all(is_denormal(v[dv]))
        assert np.array_equal(ar.bits(m[gr["m"] == 0]), ar.bits(gr["m"][gr["m"] == 0]))
    for gr, (p, m, v) in list(zip(groups, ar.expect_table(groups, **hp)))[:2]:  # (p of the update's size there)
        moved = gr["m"] != 0
        assert np.count_nonzero(ar.bits(p[moved]) != ar.bits(gr["p"][moved])) >= 0.9 * moved.sum()  # visible in p
    gr, (p, m, v) = groups[3], ar.expect_table(groups, **hp)[3]  # a denormal p moved by a denormal update
    assert np.count_nonzero(is_denormal(p) & is_denormal(gr["p"]) & (p != gr["p"])) >= 10
    # -0.0: g = -0.0 over m = v = 0 leaves m = +0.0 (0 + (-0 * c)), v = +0.0, p's bits alone
    groups, hp = T["negative_zero_grad"]
    gr, (p, m, v) = groups[0], ar.expect_table(groups, **hp)[0]
    z = ar.bits(gr["g"]) == ar.bits(F(-0.0))
    assert z.sum() >= 10 and np.all(ar.bits(m[z]) == 0) and np.all(ar.bits(v[z]) == 0)
    assert np.array_equal(ar.bits(p[z]), ar.bits(gr["p"][z]))
    # denormal g over zero moments: (1 - beta2) * g underflows to 0 or a denormal, v = 0 exactly; m is a denormal or 0
    groups, hp = T["denormal_grad"]
    gr, (p, m, v) = groups[0], ar.expect_table(groups, **hp)[0]
    assert np.all(v == 0) and np.any(is_denormal(m)) and np.all(np.abs(m) < tiny)
    # specials
    groups, hp = T["special_grad"]
    for gr, (p, m, v) in zip(groups, ar.expect_table(groups, **hp)):
        g = gr["g"]
        big = (g == F(3e38)) | (g == F(-1e25))
        assert big.sum() >= 4 and np.all(np.isposinf(v[big])) and np.all(np.isfinite(m[big]))
        assert np.array_equal(ar.bits(p[big]), ar.bits(gr["p"][big]))  # m / inf = 0: p unchanged
        ok = g == F(1e20)  # (1 - beta2) g g = 1e37 still fits
        assert ok.sum() >= 2 and np.all(np.isfinite(v[ok])) and np.all(np.isfinite(p[ok]))
        bad = np.isinf(g) | np.isnan(g)
        assert bad.sum() >= 6 and np.all(np.isnan(p[bad]))  # inf / inf
        assert np.all(np.isnan(m[np.isnan(g)])) and np.all(np.isinf(m[np.isinf(g)]))
        assert not np.any(np.isnan(p[~bad]))
    # eps = 0 over m = v = g = 0: 0 / 0
    groups, hp = T["all_zero_eps0"]
    for gr, (p, m, v) in zip(groups, ar.expect_table(groups, **hp)):
        assert np.all(np.isnan(p)) and np.all(ar.bits(m) == 0) and np.all(ar.bits(v) == 0)


def test_moment_decays_into_the_denormals_and_stays():
    """The in-view / out-of-view pattern of real training: g = 0 from step 1 on, exp_avg decays by 0.9 a step from 1e-3
    and is denormal after about 770 steps -- in the oracle it stays there, non-zero, for a hundred more."""
    m = np.array([1e-3, -1e-3], F)
    p, v = np.zeros(2, F), np.zeros(2, F)
    first = None
    for t in range(1, 900):
        p, m, v = oracle.adam_step(p, np.zeros(2, F), m, v, t, 1e-2, eps=1e-15)
        if first is None and abs(m[0]) < np.finfo(F).tiny:
            first = t
    assert 700 < first < 800 and np.all(m != 0) and np.all(np.abs(m) < np.finfo(F).tiny)
