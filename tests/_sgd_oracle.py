"""TEST INFRASTRUCTURE — numpy restatement of the fused SGD element (csrc/zs_kernels.hip sgd_elem,
torch/optim/sgd.py _single_tensor_sgd), bit for bit in fp32.

    s = gsum;  carry: s = s + carry_mul * carry
    g = s * (1/grad_div) if grad_div is a power of two else s / grad_div;  carry: carry = g
    clip: g = g * coef
    maximize: g = -g
    wd != 0:  g = fma(wd, p, g)
    momentum != 0:  buf = g if first else fma(1 - dampening, g, buf * momentum)
                    g   = fma(momentum, buf, g) if nesterov else buf
    p = fma(-lr, g, p)

``fma32`` is the exact fp32 fused multiply-add of oracle/zero_oracle.py (one copy, shared with the
Adam restatement).
"""
from __future__ import annotations

import math

import numpy as np

from oracle.zero_oracle import fma32  # noqa: F401  (re-exported: so.fma32)

F32, F64 = np.float32, np.float64


def fma32_plain(a, b, c):
    """The float64 evaluation without the residual: double rounding goes wrong at fp32 ties."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
                + np.asarray(c, F32).astype(F64)).astype(F32)


def f32_to_bf16_bits(x):
    u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def bf16_bits_to_f32(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(F32)


class SgdHP:
    """The scalars of one run, rounded to fp32 once as zs_sgd_hparams_init does."""

    def __init__(self, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, *, nesterov=False,
                 maximize=False, first=False, grad_div=1.0, carry_mul=0.0):
        self.neg_lr = F32(-float(lr))
        self.momentum = F32(momentum)
        self.omd = F32(1.0 - float(dampening))
        self.wd = F32(weight_decay)
        self.grad_div = F32(grad_div)
        self.inv_div = F32(1.0 / float(F32(grad_div)))
        self.div_pow2 = math.frexp(float(F32(grad_div)))[0] == 0.5
        self.carry_mul = F32(carry_mul)
        self.nesterov, self.maximize, self.first = bool(nesterov), bool(maximize), bool(first)


def sgd_elem(gsum, p, buf, hp: SgdHP, *, carry=None, coef=None):
    """One step over fp32 arrays; returns (p, buf, carry) as new arrays (buf / carry None when
    absent).  ``buf`` may be None on a first step (it is not read); with momentum == 0 it is
    returned as given.  ``coef``: the fp32 clip coefficient or None."""
    assert carry is None or coef is None
    with np.errstate(all="ignore"):
        s = np.asarray(gsum, F32)
        p = np.asarray(p, F32)
        if carry is not None:
            s = (s + (hp.carry_mul * np.asarray(carry, F32)).astype(F32)).astype(F32)
        g = (s * hp.inv_div).astype(F32) if hp.div_pow2 else (s / hp.grad_div).astype(F32)
        if carry is not None:
            carry = g.copy()
        if coef is not None:
            g = (g * F32(coef)).astype(F32)
        if hp.maximize:
            g = -g
        if hp.wd != 0:
            g = fma32(hp.wd, p, g)
        if hp.momentum != 0:
            assert hp.first or buf is not None
            buf = g.copy() if hp.first else fma32(hp.omd, g, (np.asarray(buf, F32) * hp.momentum).astype(F32))
            g = fma32(hp.momentum, buf, g) if hp.nesterov else buf
        p = fma32(hp.neg_lr, g, p)
    return p, buf, carry


def step_f32(p, g, buf, hp, *, carry=None, coef=None):
    """fp32 gradient, fp32 parameter: (p, buf, carry)."""
    return sgd_elem(g, p, buf, hp, carry=carry, coef=coef)


def step_bf16(master, g_bits, buf, hp, *, carry=None, coef=None):
    """bf16 gradient (uint16 bits), fp32 master with its bf16 copy: (master, p_bits, buf, carry)."""
    p, buf, carry = sgd_elem(bf16_bits_to_f32(g_bits), master, buf, hp, carry=carry, coef=coef)
    return p, f32_to_bf16_bits(p), buf, carry


def step_split(hi, lo, g_bits, buf, hp, *, carry=None, coef=None):
    """bf16 gradient, split master (oracle.c_oracle's encoding): (hi, lo, buf, carry)."""
    from oracle import c_oracle

    p, buf, carry = sgd_elem(bf16_bits_to_f32(g_bits), c_oracle.join_master(hi, lo), buf, hp,
                             carry=carry, coef=coef)
    hi, lo = c_oracle.split_master(p)
    return hi, lo, buf, carry
