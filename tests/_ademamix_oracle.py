"""TEST INFRASTRUCTURE -- numpy restatement of AdEMAMix (csrc/zs_kernels.hip AdEMAMixRule), bit for
bit in fp32, with the rounding points of DESIGN.md §4 "Fused AdEMAMix"."""
import math

import numpy as np

from _lion_oracle import bf16_bits_to_f32, f32_to_bf16_bits  # noqa: F401  (re-exported)
from oracle.zero_oracle import fma32

F32 = np.float32


class MixHP:
    # the scalars of one run, as zs_ademamix_hparams_init forms them
    def __init__(self, lr, beta1=0.9, beta2=0.999, beta3_t=0.9999, alpha_t=5.0, eps=1e-8,
                 weight_decay=0.0, step=1, *, maximize=False, grad_div=1.0, carry_mul=0.0):
        self.beta1, self.omb1 = F32(beta1), F32(1.0 - beta1)
        self.beta3, self.omb3 = F32(beta3_t), F32(1.0 - beta3_t)
        self.beta2, self.omb2 = F32(beta2), F32(1.0 - beta2)
        self.inv_bc1 = F32(1.0 / (1.0 - float(beta1) ** int(step)))
        self.alpha, self.eps = F32(alpha_t), F32(eps)
        self.bc2_sqrt = F32(math.sqrt(1.0 - float(beta2) ** int(step)))
        self.neg_lr, self.decay_mul = F32(-lr), F32(1.0 - lr * weight_decay)
        self.grad_div, self.inv_div = F32(grad_div), F32(1.0 / float(F32(grad_div)))
        self.div_pow2 = math.frexp(float(F32(grad_div)))[0] == 0.5
        self.carry_mul = F32(carry_mul)
        self.maximize = bool(maximize)


def ademamix_elem(gsum, p, m1, m2, v, hp, *, coef=None, carry=None):
    """One step over fp32 arrays (``gsum``: fp32 or bf16 codes); returns (p, m1, m2, v), with
    ``carry`` (the ZeRO-1 carry) also the new carry, the averaged gradient."""
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
        p = np.asarray(p, F32) * hp.decay_mul
        m1 = fma32(hp.omb1, g, m1 * hp.beta1)
        m2 = fma32(hp.omb3, g, m2 * hp.beta3)
        v = fma32(hp.omb2 * g, g, v * hp.beta2)
        den = np.sqrt(v) / hp.bc2_sqrt + hp.eps
        p = fma32(hp.neg_lr, fma32(hp.alpha, m2, m1 * hp.inv_bc1) / den, p)
    return (p, m1, m2, v) if carry is None else (p, m1, m2, v, new_carry.copy())
