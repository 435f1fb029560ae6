"""Fused Adam for the Gaussian parameter groups.

`FusedAdam` takes the same constructor arguments, keeps the same `param_groups` / `state` layout and
therefore the same `state_dict()` format as `torch.optim.Adam`, which is what the reference builds in
scene/gaussian_model.py:163-253 (`torch.optim.Adam(l, lr=0.0, eps=1e-15)` over named groups) and
serialises in `capture()` / `restore()`: checkpoints move in both directions.  `step()` runs ONE HIP
kernel over every group (csrc/adam.hip) instead of torch's ~10 foreach kernels per state tensor;
`step(nograd_mask=...)` also applies gui/main.py:480-513's per-Gaussian gradient mask on the fly.

Not supported (the reference uses none of them): weight_decay, amsgrad, maximize, capturable,
differentiable.  fp32 CUDA (ROCm) tensors only; there is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib


def bias_scalars(lr, beta1, beta2, t):
    """(step_size, bias_correction2_sqrt) of step t, in double, spelled as torch/optim/adam.py spells them
    (`lr / (1 - beta1**step)`, `(1 - beta2**step) ** 0.5` -- NOT math.sqrt, which differs from `** 0.5` in the last bit
    of the double at a few t); the C struct rounds each to fp32 once."""
    return lr / (1.0 - beta1 ** t), (1.0 - beta2 ** t) ** 0.5


def mask_bytes(nograd_mask, dev):
    """The [P] uint8 mask the kernel reads, on the launch device: non-zero in, non-zero out.  A cast alone would wrap
    (int64 256 -> 0) or truncate (0.5 -> 0), so every dtype but bool / uint8 goes through `!= 0`."""
    if nograd_mask.dtype not in (torch.bool, torch.uint8):
        nograd_mask = nograd_mask != 0
    return nograd_mask.to(device=dev, dtype=torch.uint8).contiguous()


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("FusedAdam covers the reference's configuration: no weight decay, no amsgrad")
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameter")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure=None, nograd_mask: torch.Tensor | None = None, skip_if: torch.Tensor | None = None):
        """One Adam update of every parameter that has a gradient.  nograd_mask: optional [P] tensor of any dtype, on any
        device; Gaussians with a non-zero entry are updated as if their gradient rows were zero.  A step that raises has
        changed nothing: no step count, no moment, no parameter.
        skip_if: optional int32[1] DEVICE tensor read by the kernel: non-zero makes this step a no-op on the device
        (parameters and both moments untouched).  Pass rasterizer.truncated_flag() to skip the view of a truncated
        speculative forward without any host round trip -- or rasterizer.truncated_flag(accumulated=True) when the step
        accumulates several views (a truncated EARLIER view must skip it too).  The skip is opt-in: without skip_if a
        truncated frame's zero gradients still move every parameter by its momentum and decay both moments.
        Known approximation: the step count lives on the host (as in torch.optim.Adam) and advances whether or not the
        device skipped, so after k skipped steps the bias corrections 1 - beta^t are those of step t rather than t - k --
        exact from a few hundred steps on (beta2^t -> 0), at most a factor 1 - beta2^(t-k) / 1 - beta2^t off before
        (k = 1 at t = 10, beta2 = 0.999: 10 % on the second-moment correction of that one step)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if nograd_mask is not None and nograd_mask.dim() != 1:
            raise ValueError("nograd_mask must be a 1-D [P] tensor")
        if skip_if is not None and (not skip_if.is_cuda or skip_if.dtype not in (torch.int32, torch.uint32)
                                    or skip_if.numel() != 1):
            raise ValueError("skip_if must be a 1-element int32 tensor on the GPU")
        lib = _lib.load()
        # Pass 1 validates EVERYTHING a launch needs and mutates nothing: a step that raises leaves every step count,
        # moment and parameter as it was (the kernel's own refusals -- 16-byte alignment -- are checked here first, so that
        # no chunk of a multi-launch step runs before a later chunk is refused).
        todo = []  # (group, p, contiguous grad, state, device pointers)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("FusedAdam: parameters must live on a ROCm GPU; there is no CPU fallback")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse:
                    raise TypeError("FusedAdam: dense float32 parameters and gradients only")
                if not p.is_contiguous():
                    raise RuntimeError("FusedAdam: parameters must be contiguous")
                if nograd_mask is not None:
                    if p.dim() == 0:
                        raise ValueError("nograd_mask: a 0-dim parameter has no per-Gaussian rows to mask")
                    if p.shape[0] != nograd_mask.shape[0]:
                        raise ValueError("nograd_mask must have one entry per Gaussian (parameter rows)")
                if skip_if is not None and skip_if.device != p.device:
                    raise ValueError("skip_if lives on another device than the parameters")
                grad = p.grad.contiguous()
                state = self.state[p]
                ptrs = [p.data_ptr(), grad.data_ptr()]
                if len(state):
                    ptrs += [state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr()]
                if (ptrs[0] | ptrs[1] | ptrs[-2] | ptrs[-1]) & 15 and p.numel():
                    raise RuntimeError("FusedAdam: tensors must be 16-byte aligned (goi_adam_step)")
                todo.append((group, p, grad, state, ptrs))
        # Pass 2: nothing below raises before the launches
        launches = {}  # (beta1, beta2, eps, device) -> list of GoiAdamGroup
        for group, p, grad, state, ptrs in todo:
            beta1, beta2 = group["betas"]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)  # torch keeps a host-side fp32 scalar
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                ptrs += [state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr()]
            state["step"] += 1
            step_size, bc2_sqrt = bias_scalars(group["lr"], beta1, beta2, float(state["step"]))
            row_len = p.numel() // p.shape[0] if p.dim() > 0 and p.shape[0] > 0 else 1
            launches.setdefault((beta1, beta2, group["eps"], p.device), []).append(_lib.GoiAdamGroup(
                ptrs[0], ptrs[1], ptrs[2], ptrs[3], p.numel(), max(row_len, 1), step_size, bc2_sqrt))
        for (beta1, beta2, eps, dev), groups in launches.items():
            # the kernel dereferences the mask on the launch device: a CPU (or other-GPU) mask is copied there, never
            # handed over as a foreign pointer
            mask = None if nograd_mask is None else mask_bytes(nograd_mask, dev)
            with torch.cuda.device(dev):
                stream = _lib.stream(dev)
                for i in range(0, len(groups), _lib.ADAM_MAX_GROUPS):
                    chunk = groups[i:i + _lib.ADAM_MAX_GROUPS]
                    arr = (_lib.GoiAdamGroup * len(chunk))(*chunk)
                    mp = _lib.ptr(mask)
                    sp = _lib.ptr(skip_if)
                    _lib.check(lib.goi_adam_step_guarded(arr, len(chunk), beta1, beta2, eps, mp, sp, stream))
        return loss
