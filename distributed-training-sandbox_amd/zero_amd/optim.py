"""Optimizers torch does not ship, in the form ``ShardedOptimizer`` wraps.

``LAMB`` (You et al. 2020, arXiv:1904.00962): Adam's direction rescaled per parameter by the trust
ratio; see the class.

``Lion`` (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms", arXiv:2302.06675): one
moment, the sign of an interpolation as the update, decoupled weight decay, no bias correction.
Its own ``step()`` is plain torch and runs on any device; handed to ``zero_amd.zero1`` / ``zero2`` /
``zero3.ShardedOptimizer`` the update runs in the fused HIP kernels instead ("Fused
Lion"), which compute what this ``step()`` computes on fp32 CPU tensors, bit for bit.

``ScheduleFreeAdamW`` (Defazio et al. 2024, "The Road Less Scheduled", arXiv:2405.15682): AdamW
without a learning-rate schedule, the gradient taken at an interpolation of the base iterate and its
running average; ``eval()`` / ``train()`` swap the parameters between the two; see the class, which
is this project's definition of the rule.

``AdEMAMix`` (Pagliardini, Ablin, Grangier 2024, "The AdEMAMix Optimizer: Better, Faster, Older",
arXiv:2409.03137): AdamW with a second, very slow EMA of the gradient mixed into the numerator, its
weight ``alpha`` and decay ``beta3`` warmed up over training (``ademamix_schedule``); see the class,
which is this project's definition of the rule.

``NorMuon`` (Li et al. 2025): Muon's orthogonalised update normalised per output neuron by a
running row second moment; see the class, which is this project's definition of the rule.

``AdamMini`` (Zhang et al. 2024): Adam's first moment per element, one second moment per block of
rows; see the class, likewise.

``Apollo`` (Zhu et al. 2024): Adam's moments on a random sign sketch of the gradient, one step scale
per channel applied to the raw gradient; see the class, likewise.
"""
from __future__ import annotations

import math

import numpy as np
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


def schedule_free_advance(group: dict):
    """Advance the host scalars of one ``ScheduleFreeAdamW`` param group by a step, in double:
    ``k`` becomes the step count ``t``, ``lr_max`` and ``weight_sum`` take this step in; returns
    ``(t, lr_t, c)``, which also stay in the group as ``lr_t`` and ``c`` (a report).  A pure
    function of the count and the group's ``lr``: every rank forms the same scalars."""
    t = int(group["k"]) + 1
    lr = group["lr"]
    lr = float(lr.item()) if torch.is_tensor(lr) else float(lr)
    warmup = int(group["warmup_steps"])
    sched = min(1.0, t / warmup) if warmup > 0 else 1.0
    lr_t = lr * sched
    lr_max = max(float(group["lr_max"]), lr_t)
    w = float(t) ** float(group["r"]) * lr_max ** float(group["weight_lr_power"])
    weight_sum = float(group["weight_sum"]) + w
    c = w / weight_sum if weight_sum != 0.0 else 0.0
    group.update(k=t, lr_max=lr_max, weight_sum=weight_sum, lr_t=lr_t, c=c)
    return t, lr_t, c


class ScheduleFreeAdamW(Optimizer):
    """``ScheduleFreeAdamW(params, lr=2.5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *,
    warmup_steps=0, r=0.0, weight_lr_power=2.0, maximize=False)``: Defazio et al. 2024, "The Road
    Less Scheduled" (arXiv:2405.15682) -- AdamW without a learning-rate schedule: the gradient is
    taken at ``y``, an interpolation of the base iterate ``z`` and the running average ``x`` of it,
    and ``x`` is what the model is evaluated at.  Adam's state: ``z`` and ``exp_avg_sq``.

    A group keeps ``k`` (steps taken), ``weight_sum``, ``lr_max`` and ``train_mode`` beside its
    options; ``state[p]`` holds ``z`` (starts as a copy of ``p``), ``exp_avg_sq`` and ``step`` (an
    fp32 CPU scalar, as torch.optim.Adam keeps it).  In train mode ``p`` holds ``y``.  One step,
    with ``t = k + 1`` and every scalar formed on the host in double (``schedule_free_advance``),
    then rounded to fp32 once where a tensor operation takes it::

        sched = min(1, t / warmup_steps) if warmup_steps > 0 else 1;   lr_t = lr * sched
        lr_max = max(lr_max, lr_t);  w = t**r * lr_max**weight_lr_power;  weight_sum += w
        c = w / weight_sum  (0 if weight_sum == 0);   bc2 = 1 - beta2**t
        a = lr_t * (beta1 * (1 - c) - 1)

        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        d = sqrt(v / bc2) + eps                        # IEEE division and root
        n = g / d;   n.add_(y, alpha=weight_decay)     # (only with weight_decay != 0)
        y.lerp_(z, c);   y.add_(n, alpha=a)
        z.add_(n, alpha=-lr_t)

    ``eval()``: ``p.lerp_(z, 1 - 1/beta1)`` (y -> x); ``train()``: ``p.lerp_(z, 1 - beta1)``
    (x -> y); both are idempotent, and ``step()`` in eval mode raises.  On fp32 parameters the
    pair returns ``y`` to within the roundings of the two lerps, not bit for bit.  Handed to
    ``zero_amd.zero1`` / ``zero2`` / ``zero3.ShardedOptimizer`` the update and the swap run in the
    fused HIP kernels instead ("Fused Schedule-Free AdamW"), which compute what this
    class computes on fp32 CPU tensors, bit for bit.
    """

    def __init__(self, params, lr: float = 2.5e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, *, warmup_steps: int = 0, r: float = 0.0,
                 weight_lr_power: float = 2.0, maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < betas[0] < 1.0:  # 0 is refused: 1 - 1/beta1 is undefined
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0 <= warmup_steps:
            raise ValueError(f"Invalid warmup_steps value: {warmup_steps}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      warmup_steps=int(warmup_steps), r=r,
                                      weight_lr_power=weight_lr_power, maximize=maximize, k=0,
                                      weight_sum=0.0, lr_max=-1.0, train_mode=True, lr_t=0.0,
                                      c=0.0))

    def _swap(self, to_eval: bool):
        for group in self.param_groups:
            if group["train_mode"] != to_eval:
                continue
            beta1 = group["betas"][0]
            weight = 1 - 1 / beta1 if to_eval else 1 - beta1
            for p in group["params"]:
                state = self.state[p]
                if "z" in state:
                    p.data.lerp_(state["z"], weight)
            group["train_mode"] = not to_eval

    @torch.no_grad()
    def eval(self):
        """The parameters to ``x``, the average (a group already there stays)."""
        self._swap(True)

    @torch.no_grad()
    def train(self):
        """The parameters back to ``y`` (a group already there stays)."""
        self._swap(False)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if not group["train_mode"]:
                raise RuntimeError("ScheduleFreeAdamW: step() in eval mode (call train() first)")
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            t, lr_t, c = schedule_free_advance(group)
            bc2 = 1 - beta2 ** t
            a = lr_t * (beta1 * (1 - c) - 1)
            for y in group["params"]:
                if y.grad is None:
                    continue
                if y.grad.is_sparse:
                    raise RuntimeError("ScheduleFreeAdamW does not support sparse gradients")
                g = -y.grad if group["maximize"] else y.grad
                state = self.state[y]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["z"] = y.detach().clone(memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(y, memory_format=torch.preserve_format)
                z, v = state["z"], state["exp_avg_sq"]
                state["step"] += 1
                v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
                # the root through float64: torch's vectorised fp32 CPU sqrt is not correctly
                # rounded, the kernel's is; the double root rounded to fp32 is (53 >= 2 * 24 + 2)
                d = v.div(bc2).to(torch.float64).sqrt_().to(v.dtype).add_(group["eps"])
                n = g.div(d)
                if group["weight_decay"] != 0:
                    n.add_(y, alpha=group["weight_decay"])
                y.lerp_(z, c)
                y.add_(n, alpha=a)
                z.add_(n, alpha=-lr_t)
        return loss


def ademamix_schedule(t: int, alpha: float, beta1: float, beta3: float, alpha_warmup=None,
                      beta3_warmup=None):
    """``(a_t, b3_t)`` of ``AdEMAMix`` at step count ``t`` (after the increment), in double: the
    paper's linear warm-up of ``alpha`` over ``alpha_warmup`` steps and its warm-up of ``beta3``
    from ``beta1``, linear in the EMA's half-life, over ``beta3_warmup`` steps; both capped at
    their final values, either constant without its warm-up.  A pure function of the count, so
    every rank and a restarted run form the same scalars."""
    a_t = float(alpha) if alpha_warmup is None else min(t * float(alpha) / alpha_warmup,
                                                        float(alpha))
    b3_t = float(beta3)
    if beta3_warmup is not None:
        s = t / beta3_warmup
        l1, l3 = math.log(beta1), math.log(beta3)
        b3_t = min(math.exp(l1 * l3 / ((1 - s) * l3 + s * l1)), float(beta3))
    return a_t, b3_t


class AdEMAMix(Optimizer):
    """``AdEMAMix(params, lr=1e-3, betas=(0.9, 0.999, 0.9999), alpha=5.0, eps=1e-8,
    weight_decay=0.0, *, alpha_warmup=None, beta3_warmup=None, maximize=False)``: Pagliardini, Ablin,
    Grangier 2024 (arXiv:2409.03137) -- AdamW whose numerator adds ``alpha`` times a slow EMA of the
    gradient (``beta3`` around 0.9999, no bias correction) to the bias-corrected fast one.

    ``state[p]`` holds ``step`` (an fp32 CPU scalar, as torch.optim.Adam keeps it), ``exp_avg``
    (fast), ``exp_avg_slow`` and ``exp_avg_sq``.  One step, with ``t = step`` after the increment
    and every scalar formed on the host in double (``a_t``, ``b3_t``: ``ademamix_schedule``), then
    rounded to fp32 once where a tensor operation takes it::

        p.mul_(1 - lr * weight_decay)
        m1.mul_(beta1).add_(g, alpha=1 - beta1)
        m2.mul_(b3_t).add_(g, alpha=1 - b3_t)
        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        den = sqrt(v) / sqrt(1 - beta2**t) + eps                 # IEEE root and division
        u = m1.mul(1 / (1 - beta1**t)).add_(m2, alpha=a_t) / den
        p.add_(u, alpha=-lr)

    Handed to ``zero_amd.zero1`` / ``zero2`` / ``zero3.ShardedOptimizer`` the update runs in the
    fused HIP kernels instead ("Fused AdEMAMix"), which compute what this ``step()``
    computes on fp32 CPU tensors, bit for bit.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999, 0.9999), alpha: float = 5.0,
                 eps: float = 1e-8, weight_decay: float = 0.0, *, alpha_warmup=None,
                 beta3_warmup=None, maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        for k in range(3):
            if not 0.0 <= betas[k] < 1.0:
                raise ValueError(f"Invalid beta parameter at index {k}: {betas[k]}")
        if not 0.0 <= alpha:
            raise ValueError(f"Invalid alpha value: {alpha}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if alpha_warmup is not None and not 0 < alpha_warmup:
            raise ValueError(f"Invalid alpha_warmup value: {alpha_warmup}")
        if beta3_warmup is not None:
            if not 0 < beta3_warmup:
                raise ValueError(f"Invalid beta3_warmup value: {beta3_warmup}")
            if not (0.0 < betas[0] and 0.0 < betas[2]):  # the schedule takes their logarithms
                raise ValueError("beta3_warmup needs beta1 > 0 and beta3 > 0 (got betas "
                                 f"{tuple(betas)})")
        super().__init__(params, dict(lr=lr, betas=betas, alpha=alpha, eps=eps,
                                      weight_decay=weight_decay, alpha_warmup=alpha_warmup,
                                      beta3_warmup=beta3_warmup, maximize=maximize))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, wd = group["lr"], group["weight_decay"]
            beta1, beta2, beta3 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("AdEMAMix does not support sparse gradients")
                g = -p.grad if group["maximize"] else p.grad
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    for name in ("exp_avg", "exp_avg_slow", "exp_avg_sq"):
                        state[name] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m1, m2, v = state["exp_avg"], state["exp_avg_slow"], state["exp_avg_sq"]
                state["step"] += 1
                t = int(state["step"])
                a_t, b3_t = ademamix_schedule(t, group["alpha"], beta1, beta3,
                                              group["alpha_warmup"], group["beta3_warmup"])
                p.mul_(1 - lr * wd)
                m1.mul_(beta1).add_(g, alpha=1 - beta1)
                m2.mul_(b3_t).add_(g, alpha=1 - b3_t)
                v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
                # the root through float64: torch's vectorised fp32 CPU sqrt is not correctly
                # rounded, the kernel's is; the double root rounded to fp32 is (53 >= 2 * 24 + 2)
                den = v.to(torch.float64).sqrt_().to(v.dtype).div_(math.sqrt(1 - beta2 ** t))
                den.add_(group["eps"])
                u = m1.mul(1 / (1 - beta1 ** t)).add_(m2, alpha=a_t).div_(den)
                p.add_(u, alpha=-lr)
        return loss


class NorMuon(Optimizer):
    """``NorMuon(params, lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True,
    ns_coefficients=<torch.optim.Muon's>, eps=1e-7, ns_steps=5, beta2=0.95, norm_eps=1e-8)``: Li et
    al. 2025, "NorMuon: Making Muon more efficient and scalable" -- Muon's orthogonalised update,
    every output neuron's row of it divided by a running second moment of that row, the whole
    rescaled so that the update's RMS is ``0.2 * lr``.  2-D parameters only, like torch's Muon.

    Per R x C parameter, with ``buf = state["momentum_buffer"]`` and ``v = state["row_exp_avg_sq"]``
    (fp32, R elements, starts at 0)::

        buf.lerp_(g, 1 - momentum);  u = g.lerp(buf, momentum) if nesterov else buf
        O  = torch.optim._muon._zeropower_via_newtonschulz(u, ns_coefficients, ns_steps, eps)
        Of = O.float()
        v.lerp_(Of.square().mean(dim=1), 1 - beta2)
        q  = v.sqrt() + norm_eps
        On = Of / q[:, None];   F = ||On||_F
        s  = 0 if F == 0 else 0.2 * lr * sqrt(R * C) / F
        p.mul_(1 - lr * weight_decay);  p.add_(On, alpha=-s)

    There is no bias correction (the rescale by ``F`` removes any global factor), no
    ``adjust_lr_fn`` (the rescale is the adjustment) and no ``step`` in the state, as torch's Muon
    keeps none.  Handed to ``zero_amd.zero2.ShardedOptimizer`` (or ``zero1`` at world size 1) the
    update runs in the fused HIP kernels instead ("Fused NorMuon").
    """

    def __init__(self, params, lr: float = 1e-3, weight_decay: float = 0.1, momentum: float = 0.95,
                 nesterov: bool = True, ns_coefficients=None, eps: float = 1e-7, ns_steps: int = 5,
                 beta2: float = 0.95, norm_eps: float = 1e-8):
        from torch.optim import _muon

        if ns_coefficients is None:
            ns_coefficients = (_muon.DEFAULT_A, _muon.DEFAULT_B, _muon.DEFAULT_C)
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 <= momentum:
            raise ValueError(f"momentum should be >= 0 but is: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight decay should be >= 0 but is: {weight_decay}")
        if not 0.0 <= beta2 < 1.0:
            raise ValueError(f"beta2 should be in [0, 1) but is: {beta2}")
        if not 0.0 <= norm_eps:
            raise ValueError(f"norm_eps should be >= 0 but is: {norm_eps}")
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, momentum=momentum,
                                      nesterov=nesterov, ns_coefficients=tuple(ns_coefficients),
                                      eps=eps, ns_steps=ns_steps, beta2=beta2, norm_eps=norm_eps))
        for group in self.param_groups:
            for p in group["params"]:
                if p.ndim != 2:
                    raise ValueError("NorMuon only supports 2D parameters whereas we found a "
                                     f"parameter with size: {p.size()}")

    @torch.no_grad()
    def step(self, closure=None):
        from torch.optim._muon import _zeropower_via_newtonschulz

        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, momentum = float(group["lr"]), group["momentum"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("NorMuon does not support sparse gradients")
                g = p.grad
                state = self.state[p]
                if "momentum_buffer" not in state:
                    state["momentum_buffer"] = torch.zeros_like(g, memory_format=torch.preserve_format)
                    state["row_exp_avg_sq"] = torch.zeros(p.shape[0], dtype=torch.float32,
                                                          device=p.device)
                buf, v = state["momentum_buffer"], state["row_exp_avg_sq"]
                buf.lerp_(g, 1 - momentum)
                u = g.lerp(buf, momentum) if group["nesterov"] else buf
                Of = _zeropower_via_newtonschulz(u, group["ns_coefficients"], group["ns_steps"],
                                                 group["eps"]).float()
                v.lerp_(Of.square().mean(dim=1), 1 - group["beta2"])
                On = Of / (v.sqrt() + group["norm_eps"])[:, None]
                F = float(torch.linalg.vector_norm(On))
                s = 0.0 if F == 0 else 0.2 * lr * (p.shape[0] * p.shape[1]) ** 0.5 / F
                p.mul_(1 - lr * group["weight_decay"])
                p.add_(On.to(p.dtype), alpha=-s)
        return loss


class LAMB(Optimizer):
    """``LAMB(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, *,
    bias_correction=True, maximize=False)``: You et al. 2020, "Large Batch Optimization for Deep
    Learning: Training BERT in 76 minutes" (arXiv:1904.00962) -- Adam's direction, rescaled per
    parameter by the trust ratio ``‖w‖ / ‖u‖``.

    Per parameter, with ``m = state["exp_avg"]``, ``v = state["exp_avg_sq"]`` and ``t`` the step
    count after the increment::

        m.lerp_(g, 1 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        u = (m / (1 - beta1**t)).div_(sqrt(v).div_(sqrt(1 - beta2**t)).add_(eps))  # IEEE sqrt
        u.add_(p, alpha=weight_decay)                  # decoupled, inside the trust ratio
        r = 1 if ‖p‖ == 0 or ‖u‖ == 0 else ‖p‖ / ‖u‖    # fp32; a NaN norm gives a NaN ratio
        p.add_(u, alpha=-(fp32(lr) * r))

    Without ``bias_correction`` both corrections are 1.  The trust ratio applies to every
    parameter of a group.  ``state[p]`` holds ``step`` (an fp32 CPU scalar, as torch.optim.Adam
    keeps it), ``exp_avg`` and ``exp_avg_sq``.  Handed to ``zero_amd.zero1`` / ``zero2`` /
    ``zero3.ShardedOptimizer`` the update runs in the fused HIP kernels instead (DESIGN.md §4,
    "Fused LAMB"), whose moments equal this ``step()``'s on fp32 CPU tensors bit for bit, and whose
    parameters do given the same ``-s``.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.0, *, bias_correction: bool = True,
                 maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      bias_correction=bool(bias_correction), maximize=maximize))
        # parameter -> the 0-d fp32 trust ratio its last step applied (a report, not state)
        self.last_trust_ratios = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("LAMB does not support sparse gradients")
                g = -p.grad if group["maximize"] else p.grad
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                state["step"] += 1
                t = float(state["step"])
                m.lerp_(g, 1 - beta1)
                v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
                bc1 = bc2_sqrt = 1.0
                if group["bias_correction"]:
                    bc1, bc2_sqrt = 1 - beta1 ** t, (1 - beta2 ** t) ** 0.5
                # the root through float64: torch's vectorised fp32 CPU sqrt is not correctly
                # rounded, the kernel's is; the double root rounded to fp32 is (53 >= 2 * 24 + 2)
                root = v.to(torch.float64).sqrt_().to(v.dtype)
                u = (m / bc1).div_(root.div_(bc2_sqrt).add_(group["eps"]))
                if group["weight_decay"] != 0:
                    u.add_(p, alpha=group["weight_decay"])
                wn = torch.linalg.vector_norm(p).to(torch.float32)
                un = torch.linalg.vector_norm(u).to(torch.float32)
                r = torch.where((wn == 0) | (un == 0), torch.ones_like(wn), wn / un)
                self.last_trust_ratios[p] = r
                s = torch.tensor(group["lr"], dtype=torch.float32, device=r.device) * r
                p.add_(u, alpha=-float(s))  # (the fp32 value, exact in a Python float)
        return loss


def adamini_blocks(shape, block_rows: int) -> int:
    """How many blocks ``AdamMini`` cuts a parameter of ``shape`` into (ValueError when
    ``block_rows`` does not divide its rows)."""
    if len(shape) < 2 or block_rows == 0:
        return 1
    rows = int(shape[0])
    if block_rows < 0 or rows % block_rows != 0:
        raise ValueError(f"AdamMini: block_rows={block_rows} does not divide the {rows} rows of a "
                         f"parameter with size: {tuple(shape)}")
    return rows // block_rows


class AdamMini(Optimizer):
    """``AdamMini(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *,
    block_rows=1, maximize=False)``: Zhang et al. 2024, "Adam-mini: Use Fewer Learning Rates To Gain
    More" (arXiv:2406.16793) -- Adam's first moment per element, one second moment per block of the
    parameter: 4 B of state per parameter plus one float per block.

    A parameter with ``ndim >= 2`` is viewed as ``R = shape[0]`` rows of ``C = numel / R`` elements
    and cut into blocks of ``block_rows`` consecutive rows (``B = R / block_rows``; it must divide
    ``R``); ``block_rows=0`` makes the whole parameter one block, and a parameter with ``ndim <= 1``
    is always one block.  ``block_rows`` is a per-group option.  Of the paper's partition,
    ``block_rows=1`` is the per-output-neuron rule of the MLP, value and projection matrices and
    the per-token rule of the embedding and output layers, ``block_rows=head_dim`` on the query and
    key matrices is the per-head rule, and ``block_rows=0`` is the whole tensor.

    Per parameter, with ``m = state["exp_avg"]``, ``v = state["block_exp_avg_sq"]`` (fp32, B
    elements, starts at 0) and ``t`` the step count after the increment::

        m.lerp_(g, 1 - beta1)
        s_b = mean over block b of g^2                      (fp32 result)
        v.mul_(beta2).add_(s, alpha=1 - beta2)
        a_b = fp32( -(lr / (1 - beta1^t)) / (sqrt(double(v_b)) / sqrt(1 - beta2^t) + eps) )
        p.mul_(1 - lr * weight_decay);   p_ij += a_b * m_ij          (block b of element ij)

    ``state[p]`` also holds ``step`` (an fp32 CPU scalar, as torch.optim.Adam keeps it).  Handed to
    ``zero_amd.zero2.ShardedOptimizer`` (or ``zero1`` at world size 1) the update runs in the fused
    HIP kernels instead ("Fused Adam-mini").
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, *, block_rows: int = 1, maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      block_rows=int(block_rows), maximize=maximize))
        for group in self.param_groups:
            for p in group["params"]:
                adamini_blocks(p.shape, group["block_rows"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr = float(group["lr"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("AdamMini does not support sparse gradients")
                g = -p.grad if group["maximize"] else p.grad
                nblk = adamini_blocks(p.shape, group["block_rows"])
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["block_exp_avg_sq"] = torch.zeros(nblk, dtype=torch.float32,
                                                            device=p.device)
                m, v = state["exp_avg"], state["block_exp_avg_sq"]
                state["step"] += 1
                t = float(state["step"])
                m.lerp_(g, 1 - beta1)
                s = g.reshape(nblk, -1).float().square().mean(dim=1)
                v.mul_(beta2).add_(s, alpha=1 - beta2)
                a = (-(lr / (1 - beta1 ** t)) /
                     (v.double().sqrt() / (1 - beta2 ** t) ** 0.5 + group["eps"])).float()
                p.mul_(1 - lr * group["weight_decay"])
                p.view(nblk, -1).add_((a[:, None] * m.reshape(nblk, -1).float()).to(p.dtype))
        return loss


def _lowbias32(x):
    """csrc/zs_sr.h's hash on a numpy uint32 array."""
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def apollo_sigma(K: int, rank: int, seed: int, epoch: int):
    """``Apollo``'s K x rank sign matrix of one (seed, epoch), fp32 +-1: zs_sr::keys and
    zs_sr::bits restated in numpy.  One hash word serves 32 consecutive k of one column."""
    seed, epoch = int(seed) % (1 << 64), int(epoch)
    u = lambda v: np.array([v & 0xFFFFFFFF], np.uint32)  # noqa: E731
    k0 = _lowbias32(u(epoch) ^ u(seed))
    k1 = _lowbias32((k0 ^ u(seed >> 32) ^ u(epoch >> 32)) + np.uint32(0x9E3779B9))
    kw = np.arange((K + 31) // 32, dtype=np.uint32)[:, None]
    j = np.arange(rank, dtype=np.uint32)[None, :]
    h = _lowbias32(kw ^ k0 ^ (j * np.uint32(0x9E3779B9))) ^ k1
    bits = (h[:, None, :] >> np.arange(32, dtype=np.uint32)[None, :, None]) & np.uint32(1)
    return 1.0 - 2.0 * bits.reshape(-1, rank)[:K].astype(np.float32)


class Apollo(Optimizer):
    """``Apollo(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *, rank=256,
    scale=1.0, scale_type="channel", update_proj_gap=200, norm_growth=1.01, seed=0,
    maximize=False)``: Zhu et al. 2024, "APOLLO: SGD-like Memory, AdamW-level Performance"
    (arXiv:2412.05270) -- Adam's moments run on a rank-``rank`` random sketch of the gradient and
    only set one step scale per channel (``scale_type="tensor"`` with ``rank=1``: per tensor,
    APOLLO-Mini), which multiplies the raw gradient.  State is ``2 rank`` floats per channel.

    2-D parameters only.  An R x C parameter has ``N = max(R, C)`` channels of ``K = min(R, C)``
    elements: its rows when ``R >= C``, its columns otherwise; ``G`` is the N x K gradient.  With
    ``q`` the parameter's ordinal in the optimizer and ``t`` the step count after the increment::

        sigma = apollo_sigma(K, rank, seed + q, (t - 1) // update_proj_gap)       (+-1, K x rank)
        S = (bf16(G) @ sigma) * fp32(1 / sqrt(rank))                             (fp32, N x rank)
        M.lerp_(S, 1 - beta1);   V = (1 - beta2) * S * S + beta2 * V
        Nh = (M / (1 - beta1^t)) / (sqrt(V) / sqrt(1 - beta2^t) + eps)
        s_c = |Nh_c| / (|S_c| + 1e-8)        (double; "tensor": both norms over the whole matrix)
        F = sqrt(sum_c s_c^2 |G_c|^2)
        lam = max(F / (F_prev + 1e-8), norm_growth) / norm_growth  if norm_growth > 0 and F_prev > 0 else 1
        F_prev = F / lam
        p = p * (1 - lr * weight_decay) - lr * sqrt(scale) * s_c / lam * g

    Two deliberate deviations from the paper: the projection is +-1 signs drawn from the counter
    hash of csrc/zs_sr.h (a Johnson-Lindenstrauss projection like the Gaussian, exact in bf16, and
    a function of indices, so no kernel ever stores it), and the sketch reads the gradient rounded
    to bf16 (``|G_c|`` and the step use the full value).  ``state[p]`` holds ``step`` (an fp32 CPU
    scalar), ``exp_avg`` and ``exp_avg_sq`` (fp32, N x rank), ``scaled_grad_norm`` (fp32, F_prev)
    and ``seed`` (int64, ``seed + q``).  Handed to ``zero_amd.zero2.ShardedOptimizer`` (or
    ``zero1`` at world size 1) the update runs in the fused HIP kernels instead (DESIGN.md §4,
    "Fused APOLLO").
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, *, rank: int = 256, scale: float = 1.0,
                 scale_type: str = "channel", update_proj_gap: int = 200,
                 norm_growth: float = 1.01, seed: int = 0, maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if int(rank) != rank or not 1 <= rank <= 256:
            raise ValueError(f"Invalid rank: {rank} (an integer in [1, 256])")
        if not 0.0 < scale:
            raise ValueError(f"Invalid scale: {scale}")
        if scale_type not in ("channel", "tensor"):
            raise ValueError(f"Invalid scale_type: {scale_type!r} ('channel' or 'tensor')")
        if int(update_proj_gap) != update_proj_gap or update_proj_gap < 1:
            raise ValueError(f"Invalid update_proj_gap: {update_proj_gap}")
        if not (norm_growth == 0 or norm_growth > 1):
            raise ValueError(f"Invalid norm_growth: {norm_growth} (0, or above 1)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      rank=int(rank), scale=scale, scale_type=scale_type,
                                      update_proj_gap=int(update_proj_gap),
                                      norm_growth=norm_growth, seed=int(seed), maximize=maximize))
        for group in self.param_groups:
            for p in group["params"]:
                if p.ndim != 2:
                    raise ValueError(f"Apollo takes 2-D parameters (got size: {tuple(p.shape)})")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        q = -1
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr, rank, ng = float(group["lr"]), group["rank"], float(group["norm_growth"])
            for p in group["params"]:
                q += 1
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Apollo does not support sparse gradients")
                g = (-p.grad if group["maximize"] else p.grad).float()
                tall = p.shape[0] >= p.shape[1]
                G = g if tall else g.t()
                N, K = G.shape
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros(N, rank, dtype=torch.float32, device=p.device)
                    state["exp_avg_sq"] = torch.zeros(N, rank, dtype=torch.float32, device=p.device)
                    state["scaled_grad_norm"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    state["seed"] = torch.tensor(group["seed"] + q, dtype=torch.int64)
                M, V = state["exp_avg"], state["exp_avg_sq"]
                state["step"] += 1
                t = float(state["step"])
                sigma = apollo_sigma(K, rank, int(state["seed"]), (int(t) - 1) // group["update_proj_gap"])
                S = (G.to(torch.bfloat16).float() @ torch.from_numpy(sigma).to(p.device)) * rank ** -0.5
                M.lerp_(S, 1 - beta1)
                V.mul_(beta2).addcmul_(S, S, value=1 - beta2)
                Nh = (M / (1 - beta1 ** t)) / (V.sqrt() / (1 - beta2 ** t) ** 0.5 + group["eps"])
                nn, ss = Nh.double().square().sum(1), S.double().square().sum(1)
                if group["scale_type"] == "tensor":
                    nn, ss = nn.sum().expand(N), ss.sum().expand(N)
                s = nn.sqrt() / (ss.sqrt() + 1e-8)
                F = float((s * s * G.double().square().sum(1)).sum().sqrt())
                Fp = float(state["scaled_grad_norm"])
                lam = max(F / (Fp + 1e-8), ng) / ng if ng > 0 and Fp > 0 else 1.0
                state["scaled_grad_norm"].fill_(F / lam)
                a = (-lr * group["scale"] ** 0.5 * s / lam).float()
                upd = a[:, None] * G
                p.mul_(1 - lr * group["weight_decay"])
                p.add_((upd if tall else upd.t()).to(p.dtype))
        return loss
