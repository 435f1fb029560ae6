"""adam_step_k (csrc/adam.hip) through goi_adam_step_guarded itself, past FusedAdam: arbitrary group tables, every tail,
mask bytes and row lengths, the skip word, hyper-parameters, value classes, refusals.  Every comparison is bit for bit
against oracle.adam_step (tests/adam_reference.py: run_table / expect_table); run_table also asserts on every call that
no word outside param / exp_avg / exp_avg_sq was written -- 16 sentinel floats on either side of each tensor, grad, the
mask, the words next to the skip flag.  tests/test_adam_reference_cpu.py shows that this gate tells an FMA from the spelled
update on these inputs, and pins what the value-class tables expect."""
import numpy as np
import pytest

from tests import adam_reference as ar

pytestmark = pytest.mark.gpu

F = np.float32
HP = dict(beta1=0.9, beta2=0.999, eps=1e-15)
MASK_BYTES = np.array([0, 1, 2, 0x80, 0xFF], np.uint8)


def check(groups, hp=HP, mask=None, what=""):
    run = ar.run_table(groups, hp["beta1"], hp["beta2"], hp["eps"], mask=mask)
    ar.assert_table(run, ar.expect_table(groups, hp["beta1"], hp["beta2"], hp["eps"], mask=mask), what)
    return run


# ---------------------------------------------------------------------------------------------------------------------
# one group, every tail


@pytest.mark.parametrize("numel", [1, 2, 3, 4, 5, 7, 8, 1020, 1021, 1022, 1023, 1024, 1025, 1027, 2047, 2048, 2049])
def test_one_group_every_tail(numel):
    gr = [ar.normal_group(numel, numel)]
    check(gr)
    # and under a mask with one byte per element (row_len = 1): the tail loop's own mask read
    mask = MASK_BYTES[np.random.default_rng(numel).integers(0, 5, numel)]
    check(gr, mask=mask)


# ---------------------------------------------------------------------------------------------------------------------
# full and ragged tables


def test_eight_groups_on_block_boundaries():
    check([ar.normal_group(1024, 100 + i, lr=1e-3 * (i + 1), t=i + 1) for i in range(8)])


def test_eight_groups_of_two_blocks_and_a_mask():
    groups = [ar.normal_group(2048, 120 + i, row_len=4, t=2 * i + 1) for i in range(8)]
    check(groups, mask=MASK_BYTES[np.random.default_rng(1).integers(0, 5, 512)])


def test_eight_groups_of_one_element():
    check([ar.normal_group(1, 200 + i, lr=1e-2 / (i + 1), t=10 * i + 1) for i in range(8)])


def test_eight_mixed_groups_each_with_its_own_scalars():
    sizes = [1025, 3, 1024, 2049, 7, 1, 4096, 1023]
    ts = [1, 2, 3, 10, 100, 1000, 30000, 7]
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 5e-3, 5e-2, 5e-3, 1e-3, 1.0]
    groups = [ar.normal_group(n, 300 + i, lr=lr, t=t) for i, (n, t, lr) in enumerate(zip(sizes, ts, lrs))]
    # the two per-group scalars really differ from group to group
    assert len({ar.scalars(g["lr"], 0.9, 0.999, g["t"]) for g in groups}) == 8
    check(groups)
    check(groups[::-1])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7])
def test_tables_of_one_to_seven_groups(n):
    sizes = [1027, 5, 1024, 2, 2050, 1021, 4]
    check([ar.normal_group(sizes[i], 400 + 10 * n + i, t=i + n) for i in range(n)])


def empty_group():
    z = np.zeros(0, F)
    return ar.group(z, z, z, z)


@pytest.mark.parametrize("where", ["first", "middle", "last", "first_and_last", "all_but_one"])
def test_zero_numel_groups_are_dropped(where):
    full = [ar.normal_group(n, 500 + i, t=i + 1) for i, n in enumerate([1025, 6, 1024])]
    e = empty_group
    groups = {"first": [e()] + full, "middle": full[:1] + [e()] + full[1:2] + [e(), e()] + full[2:],
              "last": full + [e()], "first_and_last": [e(), e()] + full + [e(), e(), e()],
              "all_but_one": [e()] * 4 + full[:1] + [e()] * 3}[where]
    run = check(groups, what=where)
    assert all(a.size == 0 for gi, g in enumerate(groups) if g["p"].size == 0 for a in run.out[gi])
    # the same with the zero-numel groups pointing at real memory instead of NULL: nothing of it is touched either
    run = ar.run_table(groups, **HP, null_empty=False)
    ar.assert_table(run, ar.expect_table(groups, **HP), where)


@pytest.mark.parametrize("n", [0, 1, 8])
def test_all_empty_table_returns_zero_and_launches_nothing(n):
    import torch
    run = ar.run_table([empty_group() for _ in range(n)], **HP, mask=np.ones(4, np.uint8), skip=0)
    assert run.rc == 0 and run.skip_after == 0
    assert torch.cuda.current_stream().query()  # nothing pending (run_table synchronised) and no error recorded


def test_more_than_eight_groups_is_refused():
    groups = [ar.normal_group(5, 600 + i) for i in range(9)]
    run = ar.run_table(groups, **HP)
    assert run.rc < 0 and "n_groups must be 0..8" in run.error
    ar.assert_unchanged(run, groups)


# ---------------------------------------------------------------------------------------------------------------------
# mask

ROW_LENS = [1, 2, 3, 4, 5, 7, 16, 45, 48]
# rows per row length, below and above one 1024-element block, chosen so that numel = P * row_len takes every residue mod 4
# the row length allows (all four for an odd one, 0 and 2 for 2, only 0 for a multiple of 4)
MASK_P = {1: [5, 6, 1027, 1028], 2: [3, 514], 3: [1, 342, 343, 344], 4: [3, 257], 5: [1, 206, 207, 208],
          7: [1, 2, 147, 148], 16: [1, 65], 45: [1, 2, 23, 24], 48: [1, 22]}


def mask_pattern(pattern, P, rng):
    on = MASK_BYTES[1:][rng.integers(0, 4, P)]  # non-zero bytes of every kind
    m = np.zeros(P, np.uint8)
    if pattern == "alternating":
        m[::2] = on[::2]
    elif pattern == "alternating_odd":
        m[1::2] = on[1::2]
    elif pattern == "first":
        m[0] = on[0]
    elif pattern == "last":
        m[-1] = on[-1]
    elif pattern == "all":
        m[:] = on
    elif pattern == "random":
        m[:] = MASK_BYTES[rng.integers(0, 5, P)]
    else:
        assert pattern == "none"
    return m


def test_mask_sizes_cover_every_residue():
    for rl, Ps in MASK_P.items():
        assert {P * rl % 4 for P in Ps} == {k * rl % 4 for k in range(4)}, rl
        assert min(Ps) * rl < 1024 < max(Ps) * rl


@pytest.mark.parametrize("row_len", ROW_LENS)
def test_mask_row_lengths_bytes_and_patterns(row_len):
    rng = np.random.default_rng(row_len)
    for P in MASK_P[row_len]:
        gr = [ar.normal_group(P * row_len, 700 + P, row_len=row_len, t=4)]
        g0 = ar.expect_table(gr, **HP)
        for pattern in ("alternating", "alternating_odd", "first", "last", "all", "none", "random"):
            mask = mask_pattern(pattern, P, rng)
            run = check(gr, mask=mask, what=(row_len, P, pattern))
            # masked rows equal the oracle with g = 0 -- momentum still moves them; unmasked rows the unmasked oracle
            em = ar.element_mask(mask, P * row_len, row_len)
            zero = dict(gr[0], g=np.zeros_like(gr[0]["g"]))
            z0 = ar.expect_table([zero], **HP)
            for got, a, b in zip(run.out[0], z0[0], g0[0]):
                ar.assert_bits(got[em], a[em], (row_len, P, pattern, "masked"))
                ar.assert_bits(got[~em], b[~em], (row_len, P, pattern, "unmasked"))
            if pattern == "all":
                assert not np.array_equal(run.out[0][0], gr[0]["p"])  # moved by momentum alone


def test_mask_over_a_table_of_different_row_lengths():
    """One [P] mask, eight groups of P rows with the reference's row lengths and one more: every group indexes the same
    bytes with its own divisor."""
    P = 259
    rls = [3, 3, 45, 16, 1, 3, 4, 7]
    groups = [ar.normal_group(P * rl, 800 + i, row_len=rl, t=i + 1) for i, rl in enumerate(rls)]
    rng = np.random.default_rng(8)
    for pattern in ("alternating", "random", "last"):
        check(groups, mask=mask_pattern(pattern, P, rng), what=pattern)


def test_a_ragged_last_row_reads_its_own_mask_byte():
    """numel need not be a multiple of row_len at the C entry: the last, partial row is row numel / row_len."""
    gr = [ar.normal_group(1030, 900, row_len=7)]  # 147 full rows and one element of row 147
    mask = np.zeros(148, np.uint8)
    mask[147] = 0x80
    check(gr, mask=mask)


# ---------------------------------------------------------------------------------------------------------------------
# skip flag

SKIP_WORDS = [0, 1, 2, 0x80000000, 0xFFFFFFFF]


def skip_table():
    return [ar.normal_group(n, 1000 + i, row_len=rl, t=i + 2) for i, (n, rl) in
            enumerate([(1025, 1), (6, 3), (1024, 4), (1, 1), (2049, 3), (3, 3), (4, 2), (1023, 3)])]


@pytest.mark.parametrize("word", SKIP_WORDS)
@pytest.mark.parametrize("masked", [False, True])
def test_skip_word(word, masked):
    groups = skip_table()
    mask = MASK_BYTES[np.random.default_rng(3).integers(0, 5, 1025)] if masked else None
    run = ar.run_table(groups, **HP, mask=mask, skip=word)
    assert run.rc == 0, run.error
    assert run.skip_after == word  # the kernel only reads it
    if word:
        ar.assert_unchanged(run, groups, hex(word))
    else:
        plain = ar.run_table(groups, **HP, mask=mask, guarded=False)
        assert plain.rc == 0, plain.error
        for a, b in zip(run.out, plain.out):
            for x, y in zip(a, b):
                assert np.array_equal(ar.bits(x), ar.bits(y))
        null = ar.run_table(groups, **HP, mask=mask, skip=None)  # a NULL flag pointer through the guarded entry
        for a, b in zip(null.out, plain.out):
            for x, y in zip(a, b):
                assert np.array_equal(ar.bits(x), ar.bits(y))
        ar.assert_table(run, ar.expect_table(groups, **HP, mask=mask))


# ---------------------------------------------------------------------------------------------------------------------
# hyper-parameters


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.0, 0.999), (0.9, 0.0), (0.5, 0.9)])
@pytest.mark.parametrize("eps", [1e-8, 1e-15, 0.0])
def test_hyper_parameters(betas, eps):
    hp = dict(beta1=betas[0], beta2=betas[1], eps=eps)
    groups = [ar.normal_group(1027, 1100 + i, lr=lr, t=t) for i, (t, lr) in
              enumerate([(1, 1e-2), (2, 5e-3), (10, 1.6e-4), (1000, 5e-2), (30000, 1e-3)])]
    # moments that are exact zeros and a zero gradient on some elements: beta = 0 and eps = 0 meet 0 / 0 there
    groups[0]["m"][::5] = 0
    groups[0]["v"][::5] = 0
    groups[0]["g"][::10] = 0
    check(groups, hp)
    check(groups, hp, mask=MASK_BYTES[np.random.default_rng(5).integers(0, 5, 1027)])


# ---------------------------------------------------------------------------------------------------------------------
# value classes

VALUE_TABLES = ar.value_class_tables()


@pytest.mark.parametrize("name", sorted(VALUE_TABLES))
def test_value_class(name):
    groups, hp = VALUE_TABLES[name]
    check(groups, hp, what=name)
    # behind a mask (odd elements see g = 0 in registers: a masked inf or NaN gradient does not reach the moments)
    mask = np.zeros(ar.VALUE_N, np.uint8)
    mask[1::2] = 0xFF
    run = check(groups, hp, mask=mask, what=name)
    if name == "special_grad":
        for gr, (p, m, v) in zip(groups, run.out):
            bad = ~np.isfinite(gr["g"])
            assert not np.any(np.isnan(m[bad & (mask != 0)])) and np.all(~np.isfinite(m[bad & (mask == 0)]))


def test_zero_gradient_decays_the_moments_into_the_denormals():
    """Forty steps with g = 0 from moments just above the smallest normal: exp_avg is denormal from the third step on and
    still non-zero at the end, on the device as in the oracle, every step bit for bit."""
    n = 39
    tiny = np.finfo(F).tiny
    m = (np.linspace(1.0, 1.3, n) * tiny * np.where(np.arange(n) % 2, -1, 1)).astype(F)
    v = (np.linspace(1.0, 1.03, n) * tiny).astype(F)
    p = ar.params_near_update(m, v, 1e-2, 0)
    z = np.zeros(n, F)
    for t in range(1, 41):
        gr = [ar.group(p, z, m, v, t=t)]
        run = check(gr, what=t)
        p, m, v = run.out[0]
    assert np.all(m != 0) and np.all(np.abs(m) < tiny) and np.all(v != 0) and np.all(v < tiny)


# ---------------------------------------------------------------------------------------------------------------------
# refusals that need a device pointer


@pytest.mark.parametrize("which", ["p", "g", "m", "v"])
@pytest.mark.parametrize("gi", [0, 2])
def test_misaligned_tensor_is_refused_and_nothing_is_touched(which, gi):
    groups = [ar.normal_group(n, 1200 + i) for i, n in enumerate([1025, 8, 7])]
    run = ar.run_table(groups, **HP, misalign=(gi, which))
    assert run.rc < 0 and run.error == ar.ALIGN_MSG, (run.rc, run.error)
    ar.assert_unchanged(run, groups, (gi, which))
