"""TEST INFRASTRUCTURE -- numpy restatement of Schedule-Free AdamW (csrc/zs_kernels.hip SfAdamRule and
sfadam_swap_kernel, zero_amd/optim.py ScheduleFreeAdamW), bit for bit in fp32: the host scalars in
double, each rounded to fp32 once, and the element with its rounding points as DESIGN.md §4 "Fused
Schedule-Free AdamW" states them (numpy's fp32 '/', '*' and sqrt are correctly rounded; ``fma32``
is the exact fma, ``lerp32`` ATen's lerp).
"""
import math

import numpy as np

from _lion_oracle import bf16_bits_to_f32, f32_to_bf16_bits  # noqa: F401  (re-exported)
from oracle.zero_oracle import fma32, lerp32

F32 = np.float32


def schedule(lr, steps, warmup_steps=0, r=0.0, weight_lr_power=2.0):
    """[(t, lr_t, c)] of the first ``steps`` steps of one param group."""
    out, weight_sum, lr_max = [], 0.0, -1.0
    for t in range(1, steps + 1):
        lr_t = lr * (min(1.0, t / warmup_steps) if warmup_steps > 0 else 1.0)
        lr_max = max(lr_max, lr_t)
        w = float(t) ** r * lr_max ** weight_lr_power
        weight_sum += w
        out.append((t, lr_t, w / weight_sum if weight_sum != 0.0 else 0.0))
    return out


class SfHP:
    """The scalars of one run, as zs_sfadam_hparams_init forms them."""

    def __init__(self, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, c=1.0, *,
                 maximize=False, grad_div=1.0, carry_mul=0.0):
        self.beta2, self.omb2 = F32(beta2), F32(1.0 - beta2)
        self.bc2 = F32(1.0 - float(beta2) ** int(step))
        self.eps, self.wd, self.c = F32(eps), F32(weight_decay), F32(c)
        self.a, self.neg_lr = F32(lr_t * (beta1 * (1.0 - c) - 1.0)), F32(-lr_t)
        self.grad_div, self.inv_div = F32(grad_div), F32(1.0 / float(F32(grad_div)))
        self.div_pow2 = math.frexp(float(F32(grad_div)))[0] == 0.5
        self.carry_mul = F32(carry_mul)
        self.maximize = bool(maximize)


def sfadam_elem(gsum, y, z, v, hp, *, coef=None, carry=None):
    """One step over fp32 arrays; ``gsum``: fp32, or bf16 codes (uint16), widened.  Returns
    (y, z, v) as new arrays; with ``carry`` (the ZeRO-1 carry: ``hp.carry_mul`` times it joins the
    sum, and the averaged gradient is the new carry) (y, z, v, carry)."""
    assert carry is None or coef is None
    gsum = np.asarray(gsum)
    s = bf16_bits_to_f32(gsum) if gsum.dtype == np.uint16 else gsum.astype(F32)
    with np.errstate(all="ignore"):
        if carry is not None:
            s = s + hp.carry_mul * np.asarray(carry, F32)
        g = s * hp.inv_div if hp.div_pow2 else s / hp.grad_div
        new_carry = g
        if coef is not None:
            g = g * F32(coef)
        if hp.maximize:
            g = -g
        v = fma32(hp.omb2 * g, g, v * hp.beta2)
        n = g / (np.sqrt(v / hp.bc2) + hp.eps)
        if hp.wd != 0:
            n = fma32(hp.wd, y, n)
        y = fma32(hp.a, n, lerp32(y, z, hp.c))
        z = fma32(hp.neg_lr, n, z)
    return (y, z, v) if carry is None else (y, z, v, new_carry.copy())


def swap(p, z, beta1, to_eval):
    """eval (y -> x) or train (x -> y) of ``p`` against ``z``."""
    return lerp32(np.asarray(p, F32), np.asarray(z, F32), 1 - 1 / beta1 if to_eval else 1 - beta1)
