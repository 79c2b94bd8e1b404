"""TEST INFRASTRUCTURE — numpy restatement of zero_amd.optim.LAMB's step and of the fused passes
(csrc/zs_lamb.hip), one fp32 operation per line of the rule in the ``LAMB`` docstring; ``fma32`` is
the exact fp32 fma of oracle/zero_oracle.py.  ``step`` takes the per-parameter ``-s`` as an input
(``neg_s``) or computes it, with the norms in float64 from the fp32 ``u`` and ``p`` (``norms64``).
"""
from __future__ import annotations

import math

import numpy as np

from oracle.zero_oracle import fma32

F32, F64 = np.float32, np.float64


class LambHP:
    """The scalars of one step at count ``t``, formed in double and rounded to fp32 once, as
    zs_lamb_hparams_init and LAMB.step() do."""

    def __init__(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, t=1, *,
                 bias_correction=True, maximize=False, grad_div=1.0):
        w = F32(1.0 - beta1)
        self.lerp_hi = not abs(w) < 0.5
        self.lerp_w = F32(w - F32(1.0)) if self.lerp_hi else w
        self.beta2, self.omb2 = F32(beta2), F32(1.0 - beta2)
        self.bc1 = F32(1.0 - beta1 ** float(t)) if bias_correction else F32(1.0)
        self.bc2_sqrt = F32((1.0 - beta2 ** float(t)) ** 0.5) if bias_correction else F32(1.0)
        self.eps, self.wd, self.lr = F32(eps), F32(weight_decay), F32(lr)
        self.grad_div = F32(grad_div)
        self.inv_div = F32(1.0 / float(F32(grad_div)))
        self.div_pow2 = math.frexp(float(F32(grad_div)))[0] == 0.5
        self.maximize = bool(maximize)


def direction(p, m, v, hp: LambHP):
    """u from the moments after their update and the parameter before its own."""
    with np.errstate(all="ignore"):
        u = (m / hp.bc1) / (np.sqrt(v) / hp.bc2_sqrt + hp.eps)
    return fma32(np.full_like(p, hp.wd), p, u) if hp.wd != 0 else u


def trust(p, u, hp: LambHP, norms64=False):
    """(wn, un, r, -s): float64 norms of the fp32 values with ``norms64`` (then r and s are float64
    too: the references of the kernel's bounds), else everything fp32."""
    if norms64:
        wn = math.sqrt(float(np.sum(p.astype(F64) ** 2)))
        un = math.sqrt(float(np.sum(u.astype(F64) ** 2)))
        r = 1.0 if wn == 0 or un == 0 else wn / un
        return wn, un, r, -(float(hp.lr) * r)
    wn, un = F32(np.linalg.norm(p)), F32(np.linalg.norm(u))
    r = F32(1.0) if wn == 0 or un == 0 else F32(wn / un)
    return wn, un, r, F32(-(hp.lr * r))


def step(p, g, m, v, hp: LambHP, *, coef=None, neg_s=None, norms64=False):
    """One step of flat fp32 arrays; returns (p, m, v, u, (wn, un, r, -s)).  ``neg_s``: apply this
    -s instead of the computed one (still returned as computed)."""
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        g = g * hp.inv_div if hp.div_pow2 else g / hp.grad_div
        if coef is not None:
            g = g * F32(coef)
        if hp.maximize:
            g = -g
        m = fma32(np.full_like(g, hp.lerp_w), g - m, g if hp.lerp_hi else m)
        v = fma32(hp.omb2 * g, g, v * hp.beta2)
    u = direction(p, m, v, hp)
    tr = trust(p, u, hp, norms64)
    ns = F32(tr[3] if neg_s is None else neg_s)
    return fma32(np.full_like(u, ns), u, p), m, v, u, tr
