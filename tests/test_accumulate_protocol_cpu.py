"""The multi-view accumulation protocol (rasterizer.accumulate_gradients + dist.accumulated_gradients, and dist.backward_views
around them) on the CPU, with the operands as the reference model hands them over: exp / sigmoid / normalize / cat / mask-multiply
of leaf parameters.  No GPU and no compiled binding: `_C.rasterize_gaussians`, `_C.rasterize_gaussians_backward`,
`_C.rasterize_gaussians_backward_accumulate` and `_C._ext` are replaced by torch stand-ins of a toy differentiable op with the
same argument lists and tuple shapes.

Everything is float64 and EXACT: the raw parameters sit where the activations and their Jacobians are dyadic (exp(0), sigmoid(0),
axis-aligned quaternions of norm 1/2, 1 or 2), the toy op is a polynomial with small integer weights, and every upstream gradient
is a small integer -- so J (g0 + g1 + g2), what the protocol computes, and J g0 + J g1 + J g2, what three serial backward() calls
leave, are the same numbers bit for bit and torch.equal is the assertion.

The per-view torch.autograd.grad of a batch hands the activations' nodes undefined gradients (the accumulating backward returns
none) and still frees what they saved; without retain_graph=True the pass at the batch's end raises "Trying to backward through
the graph a second time".  render.GaussianSet, whose parameters ARE the operands, cannot show that."""
import contextlib

import pytest
import torch
from torch import nn

from goi_hyperplane_amd import _C, dist, rasterizer
from goi_hyperplane_amd.rasterizer import GaussianRasterizationSettings

DT = torch.float64
P, M, S, H, W = 12, 4, 3, 2, 3


def _toy(view, means3D, sh, semantics, opacities, scales, rotations):
    """color [3,H,W], semantics [S,H,W], depth [1,H,W], alpha [1,H,W]: a polynomial of every operand, weighted by the integers
    of the view's 4 x 4 matrix"""
    ar = torch.arange(H * W, dtype=DT)
    pos = means3D @ view[:3, :3]
    a = opacities[:, 0] * (1 + (scales * view[3, :3]).sum(1)) + (rotations * view[:, 3]).sum(1)
    K = (torch.arange(P, dtype=DT)[:, None] + ar[None, :] * view[0, 0]) % 3 - 1 + pos[:, :1] * (ar % 2)[None, :]
    A = a[:, None] * K
    c = (sh * (1 + torch.arange(sh.shape[1], dtype=DT))[None, :, None]).sum(1)
    return ((c.T @ A).reshape(3, H, W), (semantics.T @ A).reshape(-1, H, W), (pos[:, 2][None] @ A).reshape(1, H, W),
            A.sum(0).reshape(1, H, W))


class _StandIn:
    """the three _C entries, in torch"""

    def __init__(self):
        self.batches = []  # the nine-tuples that calls with accumulate_into=None returned

    def forward(self, bg, means3D, colors, semantics, opacities, scales, rotations, scale_modifier, cov3D, viewmatrix, projmatrix,
                tanfovx, tanfovy, image_height, image_width, sh, degree, campos, prefiltered, debug):
        assert (image_height, image_width) == (H, W) and colors.numel() == 0 and cov3D.numel() == 0
        color, sem, depth, alpha = _toy(viewmatrix, means3D, sh, semantics, opacities, scales, rotations)
        radii = torch.ones(means3D.shape[0], dtype=torch.int32)
        # (the backward's argument list has no opacities: the reference keeps them in the geometry buffer)
        return 7, color, sem, depth, alpha, radii, opacities.detach().clone(), torch.zeros(1), torch.zeros(1)

    def backward_accumulate(self, accumulate_into, bg, means3D, radii, colors, semantics, scales, rotations, scale_modifier, cov3D,
                            viewmatrix, projmatrix, tanfovx, tanfovy, g_color, g_sem, g_depth, g_alpha, sh, degree, campos,
                            geomBuffer, R, binningBuffer, imageBuffer, alphas, debug):
        assert R == 7
        with torch.enable_grad():
            ops = [t.detach().clone().requires_grad_(True) for t in (means3D, sh, semantics, geomBuffer, scales, rotations)]
            outs = _toy(viewmatrix, *ops)
            pairs = [(o, g) for o, g in zip(outs, (g_color, g_sem, g_depth, g_alpha)) if g is not None]
            d_means, d_sh, d_sem, d_op, d_sc, d_rot = torch.autograd.grad([o for o, _g in pairs], ops, [g for _o, g in pairs])
        n = means3D.shape[0]
        res = (torch.zeros(n, 3, dtype=DT), torch.zeros(n, 3, dtype=DT), d_sem, d_op, d_means, torch.zeros(n, 6, dtype=DT), d_sh,
               d_sc, d_rot)
        if accumulate_into is None:
            self.batches.append(res)
            return res
        first = next(b for b in self.batches if b[4] is accumulate_into)
        for acc, t in zip(first, res):
            acc.add_(t)
        return first

    def backward(self, *args):
        return self.backward_accumulate(None, *args)


@pytest.fixture
def standin(monkeypatch):
    s = _StandIn()
    monkeypatch.setattr(_C, "rasterize_gaussians", s.forward)
    monkeypatch.setattr(_C, "rasterize_gaussians_backward", s.backward)
    monkeypatch.setattr(_C, "rasterize_gaussians_backward_accumulate", s.backward_accumulate)
    monkeypatch.setattr(_C, "_ext", lambda: s)
    monkeypatch.setitem(rasterizer._BACKWARD_MODE, "semantics_only", "auto")
    monkeypatch.setitem(rasterizer._BACKWARD_MODE, "sh_factored", False)
    monkeypatch.setitem(rasterizer._ACCUM, "state", None)
    return s


class _Model:
    """the reference GaussianModel's parameters and activations (scene/gaussian_model.py:90-123)"""

    def __init__(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        ints = lambda *shape, lo=-2, hi=3: torch.randint(lo, hi, shape, generator=g).to(DT)  # noqa: E731
        rot = torch.zeros(P, 4, dtype=DT)
        rot[torch.arange(P), torch.randint(0, 4, (P,), generator=g)] = 1.0
        rot = rot * (2.0 ** ints(P, 1, lo=-1, hi=2)) * (2 * ints(P, 1, lo=0, hi=2) - 1)  # +-(1/2, 1, 2) on one axis
        self._xyz = nn.Parameter(ints(P, 3))
        self._scaling = nn.Parameter(torch.zeros(P, 3, dtype=DT))  # exp -> 1, d exp -> 1
        self._opacity = nn.Parameter(torch.zeros(P, 1, dtype=DT))  # sigmoid -> 1/2, d sigmoid -> 1/4
        self._rotation = nn.Parameter(rot)  # normalize -> a unit axis, its Jacobian (I - q q^T) / |q|: dyadic
        self._features_dc = nn.Parameter(ints(P, 1, 3))
        self._features_rest = nn.Parameter(ints(P, M - 1, 3))
        self._semantics = nn.Parameter(ints(P, S))
        self.mask = (torch.arange(P) % 3 != 0).to(DT)[:, None]

    def parameters(self):
        return [self._xyz, self._scaling, self._opacity, self._rotation, self._features_dc, self._features_rest, self._semantics]

    def operands(self):
        return dict(means3D=self._xyz, sh=torch.cat((self._features_dc, self._features_rest), dim=1),
                    semantics=self._semantics * self.mask, opacities=torch.sigmoid(self._opacity),
                    scales=torch.exp(self._scaling), rotations=nn.functional.normalize(self._rotation))


def _settings(view):
    z = torch.zeros(3, dtype=DT)
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=1.0, tanfovy=1.0, bg=z, scale_modifier=1.0,
                                         viewmatrix=view, projmatrix=view, sh_degree=1, campos=z, prefiltered=False, debug=False)


def _views(n=3, seed=1):
    g = torch.Generator().manual_seed(seed)
    views = [torch.randint(-2, 3, (4, 4), generator=g).to(DT) for _ in range(n)]
    ups = [tuple(torch.randint(-3, 4, shape, generator=g).to(DT) for shape in ((3, H, W), (S, H, W), (1, H, W), (1, H, W)))
           for _ in range(n)]
    return views, ups


def _render(model, view):
    o = model.operands()
    sink = torch.zeros(P, 3, dtype=DT, requires_grad=True)
    color, sem, _radii, depth, alpha = rasterizer.rasterize_gaussians(
        o["means3D"], sink, o["sh"], torch.Tensor([]), o["semantics"], o["opacities"], o["scales"], o["rotations"],
        torch.Tensor([]), _settings(view))
    return dict(render=color, semantics=sem, depth=depth, alpha=alpha, viewspace_points=sink)


def _outputs(out):
    return (out["render"], out["semantics"], out["depth"], out["alpha"])


def _serial(model, views, ups):
    for p in model.parameters():
        p.grad = None
    for view, up in zip(views, ups):
        torch.autograd.backward(_outputs(_render(model, view)), up)
    assert rasterizer.last_backward_kernel() == "full"
    want = [p.grad.clone() for p in model.parameters()]
    for p in model.parameters():
        p.grad = None
    return want


def _batch(model, views, ups, retain_graph=True):
    """the protocol by hand: every view under accumulate_gradients(state), then the helper"""
    state = dict(grads=None, inputs=None, views=0)
    params = model.parameters()
    for view, up in zip(views, ups):
        with rasterizer.accumulate_gradients(state):
            out = _render(model, view)
            g = torch.autograd.grad(_outputs(out), params, up, allow_unused=True, retain_graph=retain_graph)
        assert all(t is None for t in g)  # the accumulating backward hands autograd nothing
        assert out["viewspace_points"].grad is None
        assert rasterizer.last_backward_kernel() == "full_accumulate"
    return state, dist.accumulated_gradients(state, params)


def test_three_views_through_the_activations_equal_the_serial_sum(standin):
    model = _Model()
    views, ups = _views()
    want = _serial(model, views, ups)
    assert all(float(w.abs().max()) > 0 for w in want)
    assert not bool(want[6][::3].any()) and bool(want[6][1::3].any())  # the semantic mask's rows
    state, got = _batch(model, views, ups)
    assert state["views"] == 3 and len(state["grads"]) == 9 and len(state["inputs"]) == 8
    for p, a, b in zip(model.parameters(), got, want):
        assert a.dtype == DT and a.shape == p.shape
        assert torch.equal(a, b)
    # a second batch, with a state of its own (and other upstream gradients: nothing of the first batch may linger)
    views2, ups2 = _views(seed=2)
    want2 = _serial(model, views2, ups2)
    state2, got2 = _batch(model, views2, ups2)
    assert state2["views"] == 3 and state["views"] == 3
    for a, b in zip(got2, want2):
        assert torch.equal(a, b)
    assert rasterizer._ACCUM["state"] is None


def test_a_second_batch_cannot_be_opened_while_one_is_open(standin):
    with rasterizer.accumulate_gradients(dict(grads=None, inputs=None, views=0)):
        with pytest.raises(RuntimeError, match="another batch is being accumulated"):
            with rasterizer.accumulate_gradients(dict(grads=None, inputs=None, views=0)):
                pass
    with rasterizer.accumulate_gradients(dict(grads=None, inputs=None, views=0)):  # closed again: the next one opens
        pass


def test_the_per_view_pass_must_keep_the_graph(standin):
    """what the helper's docstring says: a per-view torch.autograd.grad that frees the graph breaks the pass at the batch's end"""
    model = _Model()
    views, ups = _views()
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        _batch(model, views, ups, retain_graph=False)


@pytest.mark.parametrize("accumulate", [False, True])
def test_backward_views_on_device_equals_the_serial_sum(standin, monkeypatch, accumulate):
    """dist.backward_views itself, streams=1 (one stream: the current one, which a CPU tensor does not have -- the two stream calls
    are stood in for), on_device=True: p.grad is the serial sum, bit for bit; an extra loss term that bypasses the rasterizer
    arrives exactly once; accumulate=True adds to what is there."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: "the current stream")
    monkeypatch.setattr(torch.cuda, "stream", lambda stream: contextlib.nullcontext())
    model = _Model()
    views, ups = _views()
    want = _serial(model, views, ups)
    extra = torch.autograd.grad(4 * torch.exp(model._scaling).sum(), model._scaling)[0]
    held = [torch.full_like(p, 2.0) for p in model.parameters()]
    if accumulate:
        for p, h in zip(model.parameters(), held):
            p.grad = h.clone()

    def upstream(out, k):
        if k == 0:
            return _outputs(out) + (4 * torch.exp(model._scaling).sum(),), ups[k] + (torch.ones((), dtype=DT),)
        return _outputs(out), ups[k]
    outs = dist.backward_views(views, lambda view: _render(model, view), upstream, model.parameters(), streams=1,
                               accumulate=accumulate, on_device=True)
    assert rasterizer.last_backward_kernel() == "full_accumulate"
    assert len(outs) == 3 and all(o["viewspace_points"].grad is None for o in outs)
    for p, w, h in zip(model.parameters(), want, held):
        w = w + extra if p is model._scaling else w
        assert torch.equal(p.grad, w + h if accumulate else w)
