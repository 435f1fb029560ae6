"""FusedAdam on the GPU (csrc/adam.hip through goi_adam_step): bit-exact against the numpy oracle,
a few ulp from torch.optim.Adam running on the same device, masked step, ragged sizes."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests.test_adam_cpu import GROUPS, LRS, make_params, reference_groups

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [1, 3, 255, 1021, 4096])
def test_bit_exact_against_oracle_over_steps(P):
    from goi_hyperplane_amd.optim import FusedAdam
    params = make_params(P, device="cuda")
    opt = FusedAdam(reference_groups(params), lr=0.0, eps=1e-15)
    mine = {k: (v.detach().cpu().numpy().copy(), np.zeros(v.shape, np.float32), np.zeros(v.shape, np.float32))
            for k, v in params.items()}
    rng = np.random.default_rng(P)
    for step in range(1, 6):
        mask = (rng.random(P) < 0.3) if step % 2 == 0 else None
        for k, v in params.items():
            gr = (rng.standard_normal(v.shape) * (10.0 ** rng.integers(-6, 1))).astype(np.float32)
            v.grad = torch.from_numpy(gr).cuda()
            p, m, s = mine[k]
            mine[k] = oracle.adam_step(p, gr, m, s, step, LRS[k], eps=1e-15, nograd_rows=mask)
        opt.step(nograd_mask=None if mask is None else torch.from_numpy(mask).cuda())
        for k, v in params.items():
            st = opt.state[v]
            assert np.array_equal(v.detach().cpu().numpy(), mine[k][0]), (k, step, "param")
            assert np.array_equal(st["exp_avg"].cpu().numpy(), mine[k][1]), (k, step, "exp_avg")
            assert np.array_equal(st["exp_avg_sq"].cpu().numpy(), mine[k][2]), (k, step, "exp_avg_sq")


def test_tracks_torch_adam_on_device():
    from goi_hyperplane_amd.optim import FusedAdam
    P = 20000
    a, b = make_params(P, device="cuda"), make_params(P, device="cuda")
    fused = FusedAdam(reference_groups(a), lr=0.0, eps=1e-15)
    ref = torch.optim.Adam(reference_groups(b), lr=0.0, eps=1e-15)
    g = torch.Generator(device="cuda").manual_seed(3)
    for step in range(6):
        for k in GROUPS:
            gr = torch.randn(a[k].shape, device="cuda", generator=g) * 1e-2
            a[k].grad, b[k].grad = gr.clone(), gr.clone()
        fused.step()
        ref.step()
    for k in GROUPS:
        x, y = a[k].detach(), b[k].detach()
        assert torch.all((x - y).abs() <= 4e-7 * (y.abs() + y.abs().max())), k
        sx, sy = fused.state[a[k]], ref.state[b[k]]
        assert torch.all((sx["exp_avg"] - sy["exp_avg"]).abs() <= 4e-7 * (sy["exp_avg"].abs() + sy["exp_avg"].abs().max()))
        assert torch.all((sx["exp_avg_sq"] - sy["exp_avg_sq"]).abs() <= 4e-7 * (sy["exp_avg_sq"].abs() + sy["exp_avg_sq"].abs().max()))


def test_params_without_grad_are_skipped_and_headline_size_runs():
    from goi_hyperplane_amd.optim import FusedAdam
    P = 1_000_000
    params = make_params(P, device="cuda")
    opt = FusedAdam(reference_groups(params), lr=0.0, eps=1e-15)
    before = params["xyz"].detach().clone()
    params["semantics"].grad = torch.ones_like(params["semantics"])  # the reference's default: semantics only
    opt.step()
    assert torch.equal(params["xyz"].detach(), before) and len(opt.state[params["xyz"]]) == 0
    # first step with g = 1: m = 0.1, v = 0.001 -> p -= lr * 1 (up to rounding)
    assert torch.allclose(params["semantics"].detach() + LRS["semantics"],
                          make_params(P, device="cuda")["semantics"].detach(), atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# FusedAdam's own host path: chunked launches, launch keys, step counts, shapes, mask dtypes, refused steps, long runs.
# (The kernel itself, table by table, is in tests/test_gpu_adam_direct.py.)

from tests import adam_reference as ar  # noqa: E402

ROW_SHAPES = [(3,), (1, 3), (15, 3), (16,), (1,), (4,), (), (5,), (7,)]  # per-row shapes; () is a 1-D [P] parameter


def make_list(n, P, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn((P,) + ROW_SHAPES[i % len(ROW_SHAPES)], generator=g).cuda()) for i in range(n)]


def numpy_grads(plist, rng):
    return [np.asarray(rng.standard_normal(tuple(p.shape)) * (10.0 ** rng.integers(-6, 1)), dtype=np.float32)
            for p in plist]


class Lockstep:
    """oracle.adam_step beside an optimizer: one (param, exp_avg, exp_avg_sq, t) per tensor, each with its own t."""

    def __init__(self, plist, lr, betas=(0.9, 0.999), eps=1e-8):
        self.plist = plist
        n = len(plist)
        self.hyper = [(lr[i] if isinstance(lr, (list, tuple)) else lr, betas, eps) for i in range(n)]
        self.state = [[p.detach().cpu().numpy().copy(), np.zeros(tuple(p.shape), np.float32),
                       np.zeros(tuple(p.shape), np.float32), 0] for p in plist]

    def step(self, grads, mask=None, skipped=False):
        """grads: numpy array or None per tensor; sets .grad on the device tensors and advances the oracle (skipped: the
        step count advances, as FusedAdam documents, and nothing else)."""
        for i, (p, gr) in enumerate(zip(self.plist, grads)):
            p.grad = None if gr is None else torch.from_numpy(gr).cuda()
            if gr is None:
                continue
            st = self.state[i]
            st[3] += 1
            if skipped:
                continue
            lr, (b1, b2), eps = self.hyper[i]
            rows = None if mask is None or p.dim() == 0 else mask
            st[0], st[1], st[2] = oracle.adam_step(st[0], gr, st[1], st[2], st[3], lr, beta1=b1, beta2=b2, eps=eps,
                                                   nograd_rows=rows)

    def check(self, opt, what=""):
        for i, p in enumerate(self.plist):
            st, mine = opt.state[p], self.state[i]
            if mine[3] == 0:
                assert len(st) == 0, (what, i, "state of a parameter that never had a gradient")
                ar.assert_bits(p.detach().cpu().numpy(), mine[0], (what, i, "param"))
                continue
            assert float(st["step"]) == mine[3], (what, i, "step")
            ar.assert_bits(p.detach().cpu().numpy(), mine[0], (what, i, "param"))
            ar.assert_bits(st["exp_avg"].cpu().numpy(), mine[1], (what, i, "exp_avg"))
            ar.assert_bits(st["exp_avg_sq"].cpu().numpy(), mine[2], (what, i, "exp_avg_sq"))


@pytest.fixture
def launches(monkeypatch):
    """Counts the calls of goi_adam_step_guarded FusedAdam makes (each is one kernel launch), with their group counts."""
    from goi_hyperplane_amd import _lib
    lib = _lib.load()
    real, seen = lib.goi_adam_step_guarded, []

    def counting(arr, n, *rest):
        seen.append(n)
        return real(arr, n, *rest)
    monkeypatch.setattr(lib, "goi_adam_step_guarded", counting)
    return seen


@pytest.mark.parametrize("n,chunks", [(9, [8, 1]), (16, [8, 8]), (17, [8, 8, 1])])
@pytest.mark.parametrize("mode", ["plain", "mask", "skip_nonzero", "skip_zero"])
def test_more_than_eight_tensors_run_as_chunks(n, chunks, mode, launches):
    from goi_hyperplane_amd.optim import FusedAdam
    P = 37
    plist = make_list(n, P, n)
    opt = FusedAdam([{"params": plist}], lr=1e-2, eps=1e-15)
    ref = Lockstep(plist, 1e-2, eps=1e-15)
    rng = np.random.default_rng(n)
    for step in range(1, 4):
        mask = (rng.random(P) < 0.4) if mode == "mask" else None
        # the middle step is the guarded one: the first has created non-zero moments a skip must leave alone
        flag = None
        if mode.startswith("skip") and step == 2:
            flag = torch.tensor([0x80 if mode == "skip_nonzero" else 0], dtype=torch.int32, device="cuda")
        ref.step(numpy_grads(plist, rng), mask=mask, skipped=flag is not None and mode == "skip_nonzero")
        del launches[:]
        opt.step(nograd_mask=None if mask is None else torch.from_numpy(mask).cuda(), skip_if=flag)
        assert launches == chunks, (launches, step)
        ref.check(opt, (n, mode, step))
        if flag is not None:
            assert int(flag.item()) == (0x80 if mode == "skip_nonzero" else 0)


def test_param_groups_with_their_own_betas_and_eps_are_separate_launches(launches):
    from goi_hyperplane_amd.optim import FusedAdam
    P = 41
    plist = make_list(6, P, 2)
    hyper = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8), dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-15)]
    opt = FusedAdam([dict(params=plist[:3], **hyper[0]), dict(params=plist[3:], **hyper[1])])
    refs = [Lockstep(plist[:3], 1e-2, (0.9, 0.999), 1e-8), Lockstep(plist[3:], 1e-3, (0.5, 0.9), 1e-15)]
    rng = np.random.default_rng(2)
    for step in range(1, 4):
        mask = (rng.random(P) < 0.5) if step == 2 else None
        for r in refs:
            r.step(numpy_grads(r.plist, rng), mask=mask)
        del launches[:]
        opt.step(nograd_mask=None if mask is None else torch.from_numpy(mask).cuda())
        assert launches == [3, 3]
        for r in refs:
            r.check(opt, step)
    # same betas and eps, another lr: ONE launch (lr travels per group in the table)
    opt2 = FusedAdam([dict(params=plist[:3], lr=1e-2), dict(params=plist[3:], lr=5e-4)])
    del launches[:]
    opt2.step()
    assert launches == [6]


def test_a_parameter_without_a_gradient_on_some_steps_lags_in_t():
    from goi_hyperplane_amd.optim import FusedAdam
    plist = make_list(3, 29, 3)
    opt = FusedAdam([{"params": plist}], lr=1e-2, eps=1e-15)
    ref = Lockstep(plist, 1e-2, eps=1e-15)
    rng = np.random.default_rng(3)
    for step in range(1, 8):
        grads = numpy_grads(plist, rng)
        if step in (1, 2, 5):
            grads[1] = None  # no state at all before step 3, then t = step - 2, then step - 3
        if step == 4:
            grads[0] = None
        ref.step(grads)
        opt.step()
        ref.check(opt, step)
    assert [float(opt.state[p]["step"]) for p in plist] == [6.0, 4.0, 7.0]


def test_parameter_and_gradient_shapes():
    from goi_hyperplane_amd.optim import FusedAdam
    P = 35
    g = torch.Generator().manual_seed(4)
    plist = [torch.nn.Parameter(torch.randn((), generator=g).cuda()),          # 0-dim
             torch.nn.Parameter(torch.randn((P,), generator=g).cuda()),        # 1-D [P]
             torch.nn.Parameter(torch.randn((0, 3), generator=g).cuda()),      # no rows
             torch.nn.Parameter(torch.randn((P, 6), generator=g).cuda())]      # its gradient arrives as a strided view
    opt = FusedAdam([{"params": plist}], lr=1e-2, eps=1e-15)
    ref = Lockstep(plist, 1e-2, eps=1e-15)
    rng = np.random.default_rng(4)
    for step in range(1, 5):
        masked = step % 2 == 0
        grads = numpy_grads(plist, rng)
        mask = None
        if masked:  # a mask needs one entry per row: the 0-dim and the [0, 3] parameter sit these steps out
            grads[0] = grads[2] = None
            mask = rng.random(P) < 0.5
        ref.step(grads, mask=mask)
        wide = torch.from_numpy(np.repeat(grads[3], 2, axis=1)).cuda()
        plist[3].grad = wide[:, ::2]
        assert not plist[3].grad.is_contiguous() and torch.equal(plist[3].grad, torch.from_numpy(grads[3]).cuda())
        opt.step(nograd_mask=None if mask is None else torch.from_numpy(mask).cuda())
        ref.check(opt, step)
        assert torch.equal(wide, torch.from_numpy(np.repeat(grads[3], 2, axis=1)).cuda())  # the caller's gradient is read only
    assert float(opt.state[plist[2]]["step"]) == 2.0 and opt.state[plist[2]]["exp_avg"].shape == (0, 3)
    with pytest.raises(ValueError, match="0-dim"):
        plist[0].grad = torch.ones_like(plist[0])
        opt.step(nograd_mask=torch.zeros(P, dtype=torch.bool, device="cuda"))


MASKS = {
    "bool": lambda m: torch.from_numpy(m).cuda(),
    "uint8_twos": lambda m: torch.from_numpy(m.astype(np.uint8) * 2).cuda(),
    "uint8_mixed": lambda m: torch.from_numpy(np.where(m, np.resize(np.array([1, 2, 0x80, 0xFF], np.uint8), m.size), 0)
                                              .astype(np.uint8)).cuda(),
    "cpu_bool": lambda m: torch.from_numpy(m),
    "int64_256": lambda m: torch.from_numpy(m.astype(np.int64) * 256).cuda(),
    "int32_65536": lambda m: torch.from_numpy(m.astype(np.int32) * 65536).cuda(),
    "float_half": lambda m: torch.from_numpy(m.astype(np.float32) * 0.5).cuda(),
    "float_negative_cpu": lambda m: torch.from_numpy(m.astype(np.float64) * -1e-30),
}


@pytest.mark.parametrize("kind", sorted(MASKS))
def test_mask_dtypes_non_zero_means_masked(kind):
    from goi_hyperplane_amd.optim import FusedAdam
    P = 37
    plist = make_list(3, P, 5) + make_list(7, P, 6)[6:]  # [P,3], [P,1,3], [P,15,3] and a 1-D [P]
    opt = FusedAdam([{"params": plist}], lr=1e-2, eps=1e-15)
    ref = Lockstep(plist, 1e-2, eps=1e-15)
    rng = np.random.default_rng(5)
    for step in range(1, 4):
        mask = rng.random(P) < 0.5
        ref.step(numpy_grads(plist, rng), mask=mask)
        opt.step(nograd_mask=MASKS[kind](mask))
        ref.check(opt, (kind, step))


def snapshot(opt, plist):
    return [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}) for p in plist]


def assert_snapshot(opt, plist, snap):
    for p, (p0, st0) in zip(plist, snap):
        assert torch.equal(p.detach(), p0)
        st = opt.state[p]
        assert set(st) == set(st0), "optimizer state appeared or vanished in a refused step"
        for k in st0:
            assert torch.equal(st[k], st0[k]), k


@pytest.mark.parametrize("stepped_before", [False, True])
@pytest.mark.parametrize("fault", ["float64", "cpu", "non_contiguous", "misaligned_view", "mask_length"])
def test_a_refused_step_changes_nothing(fault, stepped_before):
    """A valid parameter FIRST, then one the step must refuse: no step count, moment or parameter moves, and no state
    appears for a parameter that had none."""
    from goi_hyperplane_amd.optim import FusedAdam
    P = 33
    good = make_list(2, P, 7)
    g = torch.Generator().manual_seed(8)
    kwargs, exc, match = {}, RuntimeError, None
    if fault == "float64":
        bad, exc, match = torch.nn.Parameter(torch.randn((P, 3), generator=g, dtype=torch.float64).cuda()), TypeError, "float32"
    elif fault == "cpu":
        bad, match = torch.nn.Parameter(torch.randn((P, 3), generator=g)), "no CPU fallback"
    elif fault == "non_contiguous":
        bad, match = torch.nn.Parameter(torch.randn((3, P), generator=g).cuda().t()), "contiguous"
    elif fault == "misaligned_view":
        base = torch.randn(P * 3 + 1, generator=g).cuda()
        bad, match = torch.nn.Parameter(base[1:].view(P, 3)), "16-byte aligned"
        assert bad.data_ptr() % 16 == 4 and bad.is_contiguous()
    else:
        bad, exc, match = torch.nn.Parameter(torch.randn((P + 1, 3), generator=g).cuda()), ValueError, "one entry per Gaussian"
        kwargs = dict(nograd_mask=torch.zeros(P, dtype=torch.bool, device="cuda"))
    plist = good + [bad]
    opt = FusedAdam([{"params": plist}], lr=1e-2, eps=1e-15)
    if stepped_before:
        for p in good:
            p.grad = torch.ones_like(p)
        opt.step()
        assert all(float(opt.state[p]["step"]) == 1.0 for p in good) and len(opt.state[bad]) == 0
    for p in plist:
        p.grad = torch.full_like(p, 0.5)
    snap = snapshot(opt, plist)
    with pytest.raises(exc, match=match):
        opt.step(**kwargs)
    torch.cuda.synchronize()
    assert_snapshot(opt, plist, snap)
    # and the optimizer is still usable: without the offender the next step is step 1 (or 2) of the good ones
    bad.grad = None
    opt.step()
    assert all(float(opt.state[p]["step"]) == (2.0 if stepped_before else 1.0) for p in good)


def test_sparse_gradients_over_a_long_run():
    """Row r sees a gradient every (r + 1)-th step and exact zeros otherwise (a Gaussian out of view): 300 steps, held to the
    oracle bit for bit every 50 and at the end."""
    from goi_hyperplane_amd.optim import FusedAdam
    P, steps = 64, 300
    plist = make_list(4, P, 9)  # [P,3], [P,1,3], [P,15,3], [P,16]
    opt = FusedAdam([{"params": plist}], lr=1e-2, eps=1e-15)
    ref = Lockstep(plist, 1e-2, eps=1e-15)
    rng = np.random.default_rng(9)
    r1 = np.arange(P) + 1
    for step in range(1, steps + 1):
        seen = step % r1 == 0
        grads = numpy_grads(plist, rng)
        for gr in grads:
            gr[~seen] = 0
        ref.step(grads)
        opt.step()
        if step % 50 == 0 or step == steps:
            ref.check(opt, step)
    assert not np.any(ref.state[0][1][P // 2:] == 0)  # rows seen once or a few times still carry a decaying moment


def test_state_dict_from_torch_adam_mid_run_continues_bit_for_bit():
    from goi_hyperplane_amd.optim import FusedAdam
    P = 33
    params = make_params(P, seed=10, device="cuda")
    plist = [params[k] for k in GROUPS]
    torch_opt = torch.optim.Adam(reference_groups(params), lr=0.0, eps=1e-15)
    rng = np.random.default_rng(10)
    for _ in range(3):
        for p, gr in zip(plist, numpy_grads(plist, rng)):
            p.grad = torch.from_numpy(gr).cuda()
        torch_opt.step()
    fused = FusedAdam(reference_groups(params), lr=0.0, eps=1e-15)
    fused.load_state_dict(torch_opt.state_dict())
    ref = Lockstep(plist, [LRS[k] for k in GROUPS], eps=1e-15)
    for p, st in zip(plist, ref.state):  # the oracle continues from torch's state
        ts = torch_opt.state[p]
        assert float(ts["step"]) == 3.0
        st[1], st[2], st[3] = ts["exp_avg"].cpu().numpy().copy(), ts["exp_avg_sq"].cpu().numpy().copy(), 3
    for step in range(4, 7):
        ref.step(numpy_grads(plist, rng))
        fused.step()
        ref.check(fused, step)
    # and back: torch.optim.Adam takes over FusedAdam's state
    back = torch.optim.Adam(reference_groups(params), lr=0.0, eps=1e-15)
    back.load_state_dict(fused.state_dict())
    assert all(float(back.state[p]["step"]) == 6.0 for p in plist)
