"""TEST INFRASTRUCTURE — numpy restatement of the fused Lion element (csrc/zs_kernels.hip LionRuleT,
zero_amd/optim.py Lion.step), bit for bit in fp32.

    s = gsum;  carry: s = s + carry_mul * carry
    g = s * (1/grad_div) if grad_div is a power of two else s / grad_div;  carry: carry = g
    clip: g = g * coef
    maximize: g = -g
    p = p * decay_mul                    decay_mul = fp32(1 - lr*wd), 1.0 when wd == 0
    c = fma(1-b1, g, m * b1)
    u = (c > 0) - (c < 0)                torch.sign: +-0 -> +0, NaN -> 0
    p = fma(-lr, u, p)
    m = fma(1-b2, g, m * b2)

``fma32`` is the exact fp32 fused multiply-add of oracle/zero_oracle.py (the double-rounding
shortcut goes wrong at ties).  bf16 momentum: the stored code is widened (exact) before the rule
and narrowed after it, to nearest even or stochastically with the low 16 bits of
``bits(e, k0, k1)`` (tests/_bf16_state_sr_oracle.py, pinned to zs_sr_bits there): the draw Adam's
exp_avg takes.
"""
from __future__ import annotations

import math

import numpy as np

from _bf16_state_sr_oracle import bits as sr_bits
from _bf16_state_sr_oracle import keys_of, sr_narrow  # noqa: F401  (re-exported: lo.keys_of)
from oracle.zero_oracle import fma32

F32, F64 = np.float32, np.float64


def f32_to_bf16_bits(x):
    u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def bf16_bits_to_f32(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(F32)


class LionHP:
    """The scalars of one run, formed in double and rounded to fp32 once, as
    zs_lion_hparams_init does."""

    def __init__(self, lr, beta1=0.9, beta2=0.99, weight_decay=0.0, *, maximize=False,
                 grad_div=1.0, carry_mul=0.0):
        lr, beta1, beta2, wd = float(lr), float(beta1), float(beta2), float(weight_decay)
        self.neg_lr = F32(-lr)
        self.beta1, self.omb1 = F32(beta1), F32(1.0 - beta1)
        self.beta2, self.omb2 = F32(beta2), F32(1.0 - beta2)
        self.decay_mul = F32(1.0 - lr * wd) if wd != 0 else F32(1.0)
        self.grad_div = F32(grad_div)
        self.inv_div = F32(1.0 / float(F32(grad_div)))
        self.div_pow2 = math.frexp(float(F32(grad_div)))[0] == 0.5
        self.carry_mul = F32(carry_mul)
        self.maximize = bool(maximize)


def sign32(c):
    """torch.sign on fp32: (c > 0) - (c < 0), so +-0 and NaN give +0."""
    c = np.asarray(c, F32)
    return (c > 0).astype(F32) - (c < 0).astype(F32)


def lion_elem(gsum, p, m, hp: LionHP, *, carry=None, coef=None):
    """One step over fp32 arrays; returns (p, m, carry) as new arrays (carry None when absent).
    ``coef``: the fp32 clip coefficient or None."""
    assert carry is None or coef is None
    with np.errstate(all="ignore"):
        s = np.asarray(gsum, F32)
        p = np.asarray(p, F32)
        m = np.asarray(m, F32)
        if carry is not None:
            s = (s + (hp.carry_mul * np.asarray(carry, F32)).astype(F32)).astype(F32)
        g = (s * hp.inv_div).astype(F32) if hp.div_pow2 else (s / hp.grad_div).astype(F32)
        if carry is not None:
            carry = g.copy()
        if coef is not None:
            g = (g * F32(coef)).astype(F32)
        if hp.maximize:
            g = -g
        p = (p * hp.decay_mul).astype(F32)
        c = fma32(hp.omb1, g, (m * hp.beta1).astype(F32))
        p = fma32(hp.neg_lr, sign32(c), p)
        m = fma32(hp.omb2, g, (m * hp.beta2).astype(F32))
    return p, m, carry


def widen_m(m):
    """The momentum as the rule sees it: fp32 as it is, bf16 codes (uint16) widened."""
    m = np.asarray(m)
    return bf16_bits_to_f32(m) if m.dtype == np.uint16 else m.astype(F32, copy=False)


def narrow_m(m_new, like, sr=None):
    """The momentum as stored: fp32 when ``like`` (the array as it was stored) is fp32; bf16 codes
    to nearest even, or with ``sr = (e, (k0, k1))`` stochastically: element ``e[i]`` of the shard's
    momentum array rounds with ``bits(e[i], k0, k1) & 0xFFFF``."""
    if np.asarray(like).dtype != np.uint16:
        assert sr is None
        return m_new
    if sr is None:
        return f32_to_bf16_bits(m_new)
    e, keys = sr
    return sr_narrow(m_new, sr_bits(np.asarray(e, np.uint64), *keys) & np.uint32(0xFFFF))


def step_f32(p, g, m, hp, *, carry=None, coef=None, sr=None):
    """fp32 gradient, fp32 parameter: (p, m, carry); ``m`` fp32, or uint16 bf16 codes."""
    p, m_new, carry = lion_elem(g, p, widen_m(m), hp, carry=carry, coef=coef)
    return p, narrow_m(m_new, m, sr), carry


def step_bf16(master, g_bits, m, hp, *, carry=None, coef=None, sr=None):
    """bf16 gradient (uint16 bits), fp32 master with its bf16 copy: (master, p_bits, m, carry)."""
    p, m_new, carry = lion_elem(bf16_bits_to_f32(g_bits), master, widen_m(m), hp, carry=carry,
                                coef=coef)
    return p, f32_to_bf16_bits(p), narrow_m(m_new, m, sr), carry


def step_split(hi, lo, g, m, hp, *, carry=None, coef=None, sr=None):
    """Split master (oracle.c_oracle's encoding); ``g``: bf16 codes (uint16) or an fp32 gradient
    (ZeRO-3's fp32 accumulation arena): (hi, lo, m, carry)."""
    from oracle import c_oracle

    g = np.asarray(g)
    gf = bf16_bits_to_f32(g) if g.dtype == np.uint16 else g.astype(F32, copy=False)
    p, m_new, carry = lion_elem(gf, c_oracle.join_master(hi, lo), widen_m(m), hp, carry=carry,
                                coef=coef)
    hi, lo = c_oracle.split_master(p)
    return hi, lo, narrow_m(m_new, m, sr), carry
