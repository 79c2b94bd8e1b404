"""Optimizers torch does not ship, in the form ``ShardedOptimizer`` wraps.

``Lion`` (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms", arXiv:2302.06675): one
moment, the sign of an interpolation as the update, decoupled weight decay, no bias correction.
Its own ``step()`` is plain torch and runs on any device; handed to ``zero_amd.zero1`` / ``zero2`` /
``zero3.ShardedOptimizer`` the update runs in the fused HIP kernels instead ("Fused
Lion"), which compute what this ``step()`` computes on fp32 CPU tensors, bit for bit.
"""
from __future__ import annotations

import torch
from torch.optim import Optimizer


class Lion(Optimizer):
    """``Lion(params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, *, maximize=False)``.

    Per parameter, with ``m = state["exp_avg"]``::

        p.mul_(1 - lr * weight_decay)
        u = m.mul(beta1).add_(g, alpha=1 - beta1).sign_()
        p.add_(u, alpha=-lr)
        m.mul_(beta2).add_(g, alpha=1 - beta2)

    ``state[p]`` holds ``step`` (an fp32 CPU scalar, as torch.optim.Adam keeps it) and ``exp_avg``.
    """

    def __init__(self, params, lr: float = 1e-4, betas=(0.9, 0.99), weight_decay: float = 0.0, *,
                 maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay,
                                      maximize=maximize))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, wd = group["lr"], group["weight_decay"]
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Lion does not support sparse gradients")
                g = -p.grad if group["maximize"] else p.grad
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m = state["exp_avg"]
                state["step"] += 1
                p.mul_(1 - lr * wd)
                u = m.mul(beta1).add_(g, alpha=1 - beta1).sign_()
                p.add_(u, alpha=-lr)
                m.mul_(beta2).add_(g, alpha=1 - beta2)
        return loss
