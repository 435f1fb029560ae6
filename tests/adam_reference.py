"""Helpers of the direct tests of the fused Adam step (csrc/adam.hip): no tests in here.

* `adam_step64`: the update in float64 (state and arithmetic), scalars formed as optim.py forms them and NOT rounded to
  fp32: the yardstick oracle.adam_step and torch.optim.Adam are measured against.
* `adam_spelled`: oracle.adam_step's fp32 arithmetic with the two per-step scalars passed in and each of the three
  updates replaceable by a mis-spelling (one FMA, a re-association): what the bit-exact gate must tell apart.
* `run_table` / `expect_table`: an arbitrary group table through goi_adam_step(_guarded) itself, past FusedAdam, every
  tensor carved out of one device buffer between sentinel words; the same table through oracle.adam_step.
* value generators for the classes the tests name.
"""
import ctypes as C

import numpy as np

from oracle import oracle

F = np.float32
SENTINEL = 0x7FA5C3A5  # a NaN pattern no update produces
PAD = 16  # sentinel floats on either side of every tensor (at least; the far side is rounded up to keep 16-byte offsets)
ALIGN_MSG = "goi_adam_step: tensors must be 16-byte aligned"
DEVICE = "cuda:0"  # where run_table puts its buffers


# ---------------------------------------------------------------------------------------------------------------------
# references


def scalars(lr, beta1, beta2, t):
    """(step_size, bc2_sqrt) in double, through optim.py's own function (what FusedAdam hands the kernel)."""
    from goi_hyperplane_amd.optim import bias_scalars
    return bias_scalars(lr, beta1, beta2, float(t))


def adam_step64(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, nograd_rows=None):
    """One Adam update in float64.  Inputs may be fp32 or float64 (a float64 run carries its own state); returns float64
    (param, exp_avg, exp_avg_sq)."""
    p, g, m, v = (np.array(a, dtype=np.float64, copy=True) for a in (param, grad, exp_avg, exp_avg_sq))
    if nograd_rows is not None:
        g[np.asarray(nograd_rows, dtype=bool)] = 0
    step_size, bc2_sqrt = scalars(lr, beta1, beta2, step)
    with np.errstate(all="ignore"):
        m = m + (g - m) * (1.0 - beta1)
        v = v * beta2 + ((1.0 - beta2) * g) * g
        den = np.sqrt(v) / bc2_sqrt + eps
        p = p - step_size * (m / den)
    return p, m, v


def fma32(a, b, c):
    """round_fp32(a * b + c) for fp32 operands: the product of two fp32 numbers is exact in double, the sum is rounded to
    double and then to fp32 (a double rounding that differs from a hardware FMA only on ties of measure zero: good enough
    to ask whether a contracted spelling can be told from the uncontracted one)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def adam_spelled(p, g, m, v, step_size, bc2_sqrt, beta1=0.9, beta2=0.999, eps=1e-8, variant=None):
    """oracle.adam_step's arithmetic on flat fp32 arrays with (step_size, bc2_sqrt) given in double (rounded to fp32 once,
    as the C struct does).  variant: None (the oracle's spelling) or one of VARIANTS."""
    p, g, m, v = (np.array(a, dtype=F, copy=True) for a in (p, g, m, v))
    omb1, b2, omb2, ssn = F(1.0 - beta1), F(beta2), F(1.0 - beta2), F(-F(step_size))
    with np.errstate(all="ignore"):
        m = fma32(g - m, omb1, m) if variant == "m_fma" else m + (g - m) * omb1
        if variant == "v_fma":
            v = fma32(omb2 * g, g, v * b2)
        elif variant == "v_reassoc":
            v = b2 * v + omb2 * (g * g)
        else:
            v = v * b2 + (omb2 * g) * g
        den = np.sqrt(v) / F(bc2_sqrt) + F(eps)
        p = fma32(ssn, m / den, p) if variant == "p_fma" else p + ssn * (m / den)
    return p, m, v


VARIANTS = {"m_fma": 1, "v_fma": 2, "v_reassoc": 2, "p_fma": 0}  # name -> index of the tensor it touches in (p, m, v)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def assert_bits(got, ref, what=""):
    """Bit for bit: NaN exactly where the reference has NaN, every other element equal as int32 (so -0.0 != 0.0 and a
    flushed denormal shows)."""
    got, ref = np.asarray(got, F).reshape(-1), np.asarray(ref, F).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ng, nr = np.isnan(got), np.isnan(ref)
    assert np.array_equal(ng, nr), (what, "NaN positions", np.flatnonzero(ng != nr)[:8])
    bad = np.flatnonzero((bits(got) != bits(ref)) & ~nr)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], ref[bad[:8]])


# ---------------------------------------------------------------------------------------------------------------------
# tables


def group(p, g, m, v, row_len=1, lr=1e-2, t=1):
    """One entry of a table: four flat fp32 arrays of one length (0 allowed), the row length the mask is indexed with,
    and the (lr, t) the two per-group scalars are formed from."""
    p, g, m, v = (np.ascontiguousarray(a, dtype=F).reshape(-1) for a in (p, g, m, v))
    assert p.size == g.size == m.size == v.size
    return dict(p=p, g=g, m=m, v=v, row_len=int(row_len), lr=float(lr), t=int(t))


def element_mask(mask, numel, row_len):
    """The mask as the kernel reads it for element e: byte e / row_len, non-zero masks."""
    return np.asarray(mask)[np.arange(numel) // row_len] != 0


def expect_table(groups, beta1, beta2, eps, mask=None):
    """[(p, m, v)] per group through oracle.adam_step; each group with its own step_size, bc2_sqrt and row_len."""
    out = []
    for gr in groups:
        rows = None if mask is None else element_mask(mask, gr["p"].size, gr["row_len"])
        with np.errstate(all="ignore"):
            out.append(oracle.adam_step(gr["p"], gr["g"], gr["m"], gr["v"], gr["t"], gr["lr"], beta1=beta1, beta2=beta2,
                                        eps=eps, nograd_rows=rows))
    return out


class TableRun:
    """What run_table returns: rc / error of the C entry, [(p, m, v)] per group as read back, the skip word after."""

    def __init__(self, rc, error, out, skip_after):
        self.rc, self.error, self.out, self.skip_after = rc, error, out, skip_after


def run_table(groups, beta1, beta2, eps, mask=None, skip=None, guarded=True, misalign=None, null_empty=True):
    """The table through goi_adam_step_guarded (guarded=False: goi_adam_step; skip must be None then) on cuda:0.
    mask: uint8 array or None; skip: the 32-bit flag word as an int, or None for a NULL flag pointer.
    misalign: (group index, "p"|"g"|"m"|"v"): that pointer is handed over 4 bytes further on.
    null_empty: zero-numel groups get NULL pointers.
    Asserts, whatever the call returns: every sentinel word of the float buffer, the mask buffer and around the flag word
    is untouched, grad and the mask are unchanged bit for bit."""
    import torch

    from goi_hyperplane_amd import _lib
    lib = _lib.load()
    dev = torch.device(DEVICE)
    # layout, in floats: PAD | tensor | round up to 4 | PAD | tensor ...
    offs, cur = [], PAD
    for gr in groups:
        o = {}
        for k in "pgmv":
            o[k] = cur
            cur += (gr["p"].size + 3) // 4 * 4 + PAD
        offs.append(o)
    img = np.full(cur, SENTINEL, np.int32)
    is_out = np.zeros(cur, bool)  # words the kernel may write
    for gr, o in zip(groups, offs):
        n = gr["p"].size
        for k in "pgmv":
            img[o[k]:o[k] + n] = bits(gr[k])
            if k != "g":
                is_out[o[k]:o[k] + n] = True
    buf = torch.from_numpy(img.copy()).to(dev)
    assert buf.data_ptr() % 16 == 0
    mimg = mbuf = None
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        for gr in groups:  # every byte the kernel can index exists
            assert gr["p"].size == 0 or (gr["p"].size - 1) // gr["row_len"] < mask.size
        mimg = np.full(mask.size + 128, 0xA5, np.uint8)
        mimg[64:64 + mask.size] = mask
        mbuf = torch.from_numpy(mimg.copy()).to(dev)
    simg = np.full(2 * PAD + 1, SENTINEL, np.int32)
    sbuf = None
    if skip is not None:
        simg[PAD] = np.array([skip & 0xFFFFFFFF], np.uint32).view(np.int32)[0]
        sbuf = torch.from_numpy(simg.copy()).to(dev)

    def at(gi, k):
        if groups[gi]["p"].size == 0 and null_empty:
            return None
        return buf.data_ptr() + 4 * offs[gi][k] + (4 if misalign == (gi, k) else 0)

    rows = []
    for gi, gr in enumerate(groups):
        step_size, bc2_sqrt = scalars(gr["lr"], beta1, beta2, gr["t"])
        rows.append(_lib.GoiAdamGroup(at(gi, "p"), at(gi, "g"), at(gi, "m"), at(gi, "v"), gr["p"].size, gr["row_len"],
                                      step_size, bc2_sqrt))
    arr = (_lib.GoiAdamGroup * max(len(rows), 1))(*rows)
    mp = None if mbuf is None else C.c_void_p(mbuf.data_ptr() + 64)
    with torch.cuda.device(dev):
        stream = _lib.stream(dev)
        if guarded:
            sp = None if sbuf is None else C.c_void_p(sbuf.data_ptr() + 4 * PAD)
            rc = lib.goi_adam_step_guarded(arr, len(rows), beta1, beta2, eps, mp, sp, stream)
        else:
            assert skip is None
            rc = lib.goi_adam_step(arr, len(rows), beta1, beta2, eps, mp, stream)
        error = _lib.last_error() if rc < 0 else ""
        torch.cuda.synchronize(dev)
    got = buf.cpu().numpy()
    touched = np.flatnonzero(~is_out & (got != img))
    assert touched.size == 0, ("a sentinel or grad word was written", touched[:8], [hex(x & 0xFFFFFFFF) for x in got[touched[:8]]])
    if mbuf is not None:
        assert np.array_equal(mbuf.cpu().numpy(), mimg), "the mask buffer was written"
    skip_after = None
    if sbuf is not None:
        sgot = sbuf.cpu().numpy()
        assert np.array_equal(np.delete(sgot, PAD), np.delete(simg, PAD)), "a word next to the skip flag was written"
        skip_after = int(sgot[PAD:PAD + 1].view(np.uint32)[0])
    out = [tuple(got[o[k]:o[k] + gr["p"].size].view(F).copy() for k in "pmv") for gr, o in zip(groups, offs)]
    return TableRun(rc, error, out, skip_after)


def assert_table(run, want, what=""):
    assert run.rc == 0, (what, run.rc, run.error)
    assert len(run.out) == len(want)
    for gi, (got, ref) in enumerate(zip(run.out, want)):
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, ref):
            assert_bits(a, b, (what, "group", gi, name))


def assert_unchanged(run, groups, what=""):
    for gi, (got, gr) in enumerate(zip(run.out, groups)):
        for name, a, k in zip(("param", "exp_avg", "exp_avg_sq"), got, "pmv"):
            assert np.array_equal(bits(a), bits(gr[k])), (what, "group", gi, name)


# ---------------------------------------------------------------------------------------------------------------------
# value generators (all return fp32)


def normal_inputs(n, seed, t=1):
    """(p, g, m, v) of the distribution tests/test_gpu_adam.py steps through: p ~ N(0,1), g ~ N(0,1) * 10^k with k in
    -6..0 (here per element, so one small tensor sees every magnitude), and moments as a few such steps leave them: m of
    the gradient's magnitude, v of its square."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.integers(-6, 1, n)
    p = rng.standard_normal(n)
    g = rng.standard_normal(n) * scale
    m = 0.3 * rng.standard_normal(n) * scale
    v = (0.01 + rng.random(n)) * scale * scale * 0.05
    return tuple(a.astype(F) for a in (p, g, m, v))


def normal_group(n, seed, row_len=1, lr=1e-2, t=3):
    return group(*normal_inputs(n, seed), row_len=row_len, lr=lr, t=t)


def denormals(n, seed, signed=True):
    """Magnitudes 1e-39 .. 1e-45, log-uniform (below 1.18e-38 every fp32 is denormal; 1e-45 rounds to the smallest one)."""
    rng = np.random.default_rng(seed)
    a = 10.0 ** rng.uniform(-45.0, -39.0, n)
    a[0], a[-1] = 1e-39, 1.4e-45
    if signed:
        a *= rng.choice([-1.0, 1.0], n)
    out = a.astype(F)
    assert np.all(out != 0) and np.all(np.abs(out) < np.finfo(F).tiny)
    return out


def small_params(n, seed):
    """Parameters of magnitude 1e-42 .. 1e-3 (log-uniform, signed, with an exact zero and a -0.0): small enough for the
    update a denormal moment gives (1e-22 and less) to show in their bits."""
    rng = np.random.default_rng(seed)
    a = (10.0 ** rng.uniform(-42.0, -3.0, n) * rng.choice([-1.0, 1.0], n)).astype(F)
    a[n // 2], a[n // 2 + 1] = 0.0, -0.0
    return a


def params_near_update(m, v, lr, seed):
    """Parameters of the size of the update (lr |m| / sqrt(v), up to the bias corrections) and up to eight times it, either
    sign, so that the update shows in their bits however small the moments are; zero where the update is."""
    upd = lr * np.abs(m.astype(np.float64)) / (np.sqrt(v.astype(np.float64)) + 1e-15)
    return (upd * np.random.default_rng(seed).uniform(-8.0, 8.0, m.size)).astype(F)


def normals(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F)


VALUE_N = 39  # nine float4s and a three-element tail
VALUE_HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-15)
SPECIALS = np.array([np.inf, np.nan, 3e38, 1e20, -1e25, -np.inf], dtype=F)


def value_class_tables():
    """name -> (groups, hyper-parameters): one small table per value class, shared by the CPU pins (oracle against
    adam_step64) and the GPU test (kernel against oracle)."""
    n, z = VALUE_N, np.zeros(VALUE_N, F)
    third = np.arange(n) % 3
    seeded_m = np.where(third == 0, normals(n, 1, 1e-3), np.where(third == 1, denormals(n, 2), 0)).astype(F)
    # shifted by one so that (m, v) meets as (normal, zero), (denormal, normal), (zero, denormal) and, in the second
    # group, every other pairing
    seeded_v = np.abs(np.roll(seeded_m, 1)).astype(F)
    seeded_v2 = np.abs(np.roll(seeded_m, 2)).astype(F)
    neg0 = np.where(third == 0, F(-0.0), np.where(third == 1, F(0.0), normals(n, 3, 1e-4))).astype(F)
    g_special = normals(n, 4, 1e-2)
    g_special[::2] = np.resize(SPECIALS, (n + 1) // 2)
    tables = {
        "zero_grad_seeded_moments": [group(params_near_update(seeded_m, seeded_v, 1e-2, 10), z, seeded_m, seeded_v),
                                     group(params_near_update(seeded_m, seeded_v2, 1e-3, 11), z, seeded_m, seeded_v2,
                                           lr=1e-3, t=1000),
                                     group(small_params(n, 12), z, seeded_m, np.abs(seeded_m)),
                                     # a denormal update (lr m / sqrt(v), v = 1) of a denormal parameter
                                     group(params_near_update(denormals(n, 36), np.ones(n, F), 0.5, 37), z,
                                           denormals(n, 36), np.ones(n, F), lr=0.5, t=1000)],
        "negative_zero_grad": [group(small_params(n, 13), neg0, z, z),
                               group(small_params(n, 14), neg0, np.roll(neg0, 1), z),
                               group(small_params(n, 15), neg0, -neg0, np.abs(normals(n, 5, 1e-6)))],
        "denormal_grad": [group(small_params(n, 16), denormals(n, 6), z, z),
                          group(small_params(n, 17), denormals(n, 7), denormals(n, 8), np.abs(denormals(n, 9))),
                          group(small_params(n, 18), denormals(n, 20), normals(n, 21, 1e-3), np.abs(normals(n, 22, 1e-6)))],
        "special_grad": [group(normals(n, 23), g_special, normals(n, 24, 1e-2), np.abs(normals(n, 25, 1e-4))),
                         group(small_params(n, 26), np.roll(g_special, 1), z, z)],
        "denormal_v_normal_m": [group(small_params(n, 27), normals(n, 28, 1e-30), normals(n, 29, 1e-3),
                                      np.abs(denormals(n, 30))),
                                group(normals(n, 31), z, normals(n, 32), np.abs(denormals(n, 33)))],
    }
    out = {k: (v, dict(VALUE_HYPER)) for k, v in tables.items()}
    # eps = 0 over m = v = g = 0: 0 / 0
    out["all_zero_eps0"] = ([group(small_params(n, 34), z, z, z), group(normals(n, 35), z, z, z, t=7)],
                            dict(beta1=0.9, beta2=0.999, eps=0.0))
    return out
