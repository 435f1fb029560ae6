"""Named cases for goi_mcmc_relocate / goi_mcmc_noise: inputs only, generated from seeds; tests/test_mcmc_cpu.py holds the list
to the coverage the feature was specified with, tests/test_gpu_mcmc.py runs every one of them against tests/mcmc_reference.py.

A case is a dict: P, rest (floats per f_rest row: 0 or 45), S, opacity [P] float32 ACTIVATED, draws (list of ints),
selection ([P] uint8 or None), min_opacity, max_moves, frac (num, den), n_max, moments (names of the groups that have Adam
moments)."""
import numpy as np

NAMES = ("xyz", "f_dc", "f_rest", "semantics", "opacity", "scaling", "rotation")
MIN_OP = float(np.float32(0.005))
NO_LIMIT = (1 << 32, 1)
U_MAX = 2 ** 32 - 1


def _case(opacity, draws, *, rest=45, S=16, selection=None, min_opacity=MIN_OP, max_moves=None, frac=NO_LIMIT, n_max=51,
          moments=NAMES):
    opacity = np.asarray(opacity, np.float32)
    P = int(opacity.shape[0])
    return {"P": P, "rest": rest, "S": S, "opacity": opacity, "draws": [int(u) for u in draws],
            "selection": None if selection is None else np.asarray(selection, np.uint8), "min_opacity": min_opacity,
            "max_moves": P if max_moves is None else max_moves, "frac": frac, "n_max": n_max, "moments": tuple(moments)}


def _mixed(P, seed, dead_share=0.3):
    """dead and alive interleaved at random: dead opacities in (0, 0.005), alive ones in (0.01, 0.999)"""
    rng = np.random.default_rng(seed)
    dead = rng.random(P) < dead_share
    op = np.where(dead, rng.random(P) * 0.004 + 0.0005, rng.random(P) * 0.989 + 0.01).astype(np.float32)
    return op, rng


def _draws(rng, n):
    return rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).tolist()


def _sized(P, seed, rest, S):
    op, rng = _mixed(P, seed)
    return _case(op, _draws(rng, P), rest=rest, S=S)


def _power_of_two():
    """8 alive rows of opacity 0.5 (w = 2^23, T = 2^26, t = u >> 6) between dead ones: draws that land on C_i - 1 and on C_i"""
    op = np.full(24, 0.001, np.float32)
    alive = [1, 2, 5, 8, 9, 13, 20, 23]
    op[alive] = 0.5
    draws = []
    for n in range(1, 8):  # C = n * 2^23
        C = n << 23
        draws += [(C << 6) - 1, C << 6]  # t = C - 1: still row n - 1;  t = C: row n
    return _case(op, draws + [0, U_MAX], rest=0, S=1)


def _one_alive():
    op = np.full(301, 0.002, np.float32)
    op[150] = 0.9
    return _case(op, _draws(np.random.default_rng(7), 300), rest=0, S=1)


def _block():
    op, rng = _mixed(257, 11, dead_share=0.0)
    op[100:140] = 0.001
    return _case(op, _draws(rng, 40))


def _interleaved():
    op = np.where(np.arange(257) % 2 == 0, 0.002, 0.6).astype(np.float32)
    return _case(op, _draws(np.random.default_rng(12), 257), S=1)


def _threshold():
    """opacity exactly min_opacity is dead, the next float above it alive"""
    op, rng = _mixed(65, 13)
    op[3] = np.float32(MIN_OP)
    op[4] = np.nextafter(np.float32(MIN_OP), np.float32(1.0))
    op[5] = np.float32(MIN_OP)
    return _case(op, _draws(rng, 65), rest=0)


def _opaque():
    """a source of opacity 1.0 (clamped at 1 - 2^-24) and one above 1"""
    op = np.array([1.0, 0.001, 0.001, 0.002, 1.0, 0.003, 1.5, 0.001], np.float32)
    return _case(op, [0, U_MAX, 1 << 31, 1 << 30, 3 << 30], rest=0, S=1)


def _nan():
    op, rng = _mixed(65, 14)
    op[[0, 7, 64]] = np.nan
    return _case(op, _draws(rng, 65), S=1)


def _frozen_dead():
    op, rng = _mixed(65, 15)
    sel = np.ones(65, np.uint8)
    op[[2, 9]] = 0.001
    sel[[2, 9, 30]] = 0
    return _case(op, _draws(rng, 65), selection=sel)


def _frozen_only_source():
    op = np.full(10, 0.001, np.float32)
    op[4] = 0.8
    sel = np.ones(10, np.uint8)
    sel[4] = 0
    return _case(op, _draws(np.random.default_rng(16), 10), selection=sel, rest=0, S=1)


def _with(base, **kw):
    c = dict(base)
    c.update(kw)
    return c


def _n_dead(c):
    sel = np.ones(c["P"], bool) if c["selection"] is None else c["selection"] != 0
    with np.errstate(invalid="ignore"):
        return int((sel & (c["opacity"].astype(np.float64) <= c["min_opacity"])).sum())


def _n_alive(c):
    sel = np.ones(c["P"], bool) if c["selection"] is None else c["selection"] != 0
    with np.errstate(invalid="ignore"):
        return int((sel & (c["opacity"].astype(np.float64) > c["min_opacity"])).sum())


def cases():
    """{name: case}, built afresh on every call (nothing shared is mutable state)"""
    out = {
        "p0": _case(np.zeros(0, np.float32), [], rest=0, S=1),
        "p1_alive": _case([0.5], [5], rest=45, S=1),
        "p1_dead": _case([0.001], [5], rest=0, S=16),
        "p2": _case([0.001, 0.7], [123456789, 1], rest=45, S=16),
        "p63": _sized(63, 1, 0, 1),
        "p64": _sized(64, 2, 45, 16),
        "p65": _sized(65, 3, 0, 16),
        "p257": _sized(257, 4, 45, 1),
        "p5000": _sized(5000, 5, 45, 16),
        "no_dead": _case(_mixed(65, 6, dead_share=0.0)[0], _draws(np.random.default_rng(6), 65)),
        "all_dead": _case(np.full(64, 0.001, np.float32), _draws(np.random.default_rng(8), 64), rest=0),
        "one_alive_300_dead": _one_alive(),
        "interleaved": _interleaved(),
        "dead_block": _block(),
        "boundaries": _power_of_two(),
        "threshold": _threshold(),
        "opaque": _opaque(),
        "nan": _nan(),
        "frozen_dead": _frozen_dead(),
        "frozen_only_source": _frozen_only_source(),
    }
    base = out["p257"]
    nd, na = _n_dead(base), _n_alive(base)
    out["u_zero"] = _with(base, draws=[0] * 257)
    out["u_max"] = _with(base, draws=[U_MAX] * 257)
    out["more_draws"] = _with(base, draws=base["draws"] + base["draws"][::-1])
    out["fewer_draws"] = _with(base, draws=base["draws"][:nd // 2])
    out["max_moves_0"] = _with(base, max_moves=0)
    out["max_moves_1"] = _with(base, max_moves=1)
    out["max_moves_below"] = _with(base, max_moves=nd - 1)
    out["max_moves_above"] = _with(base, max_moves=nd + 5)
    out["frac_to_0"] = _with(base, frac=(1, na + 1))
    out["frac_to_1"] = _with(base, frac=(1, na))
    out["frac_5_percent"] = _with(out["p5000"], frac=(1, 20))
    out["moments_some"] = _with(out["p65"], moments=("xyz", "opacity", "f_rest"))
    out["moments_none"] = _with(out["p64"], moments=())
    out["n_max_3"] = _with(out["one_alive_300_dead"], n_max=3)
    return out


def row_lens(c):
    return {"xyz": 3, "f_dc": 3, "f_rest": c["rest"], "semantics": c["S"], "opacity": 1, "scaling": 3, "rotation": 4}


def tensors(c, seed=0):
    """{name: float32 [P, row_len]} parameters and {name: (exp_avg, exp_avg_sq)} moments of a case, seeded"""
    rng = np.random.default_rng(1000 + seed)
    P = c["P"]
    params = {n: rng.standard_normal((P, rl)).astype(np.float32) for n, rl in row_lens(c).items()}
    params["scaling"] = (params["scaling"] * 0.5 - 3.0).astype(np.float32)
    moments = {n: (rng.standard_normal(params[n].shape).astype(np.float32), rng.random(params[n].shape).astype(np.float32))
               for n in c["moments"]}
    return params, moments
