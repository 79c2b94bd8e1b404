"""numpy restatement of the sharded EMA (zs_adamset_run_ema) and its composition with the existing
Adam oracles (no GPU needed; tests/test_ema_oracle.py pins it against torch's CPU arithmetic).

One EMA step is ATen's lerp, ``ema = lerp(ema, master_after, fp32(1 - decay))``, which
oracle/zero_oracle.py already restates for exp_avg (``lerp32``).  ``master_after`` is the fp32 master
as the update stored it: for the split master the join of the ``hi`` / ``lo`` words written, which at
an exact tie is 1 ulp from the computed value.

The composed updates take the gradient the element rule sees, ``g_eff`` (fp32: the reduced sum
divided by the world size, times the clip coefficient when there is one; ``prep``), and run the C
oracle's fp32 update with a divisor of 1 on the fp32 master, then store it the way the kernel does.
The existing oracles are not touched.
"""
import numpy as np

from oracle import c_oracle
from oracle import zero_oracle as zo

F32 = np.float32
DECAYS = (0.999, 0.9999, 0.99, 0.9, 0.5, 0.3, 0.0, 1.0)

assert F32(2.0 ** -149) + F32(2.0 ** -149) == 2.0 ** -148, "numpy flushed a denormal"


def weight(decay) -> np.float32:
    """fp32(1 - decay), the subtraction in double."""
    return F32(1.0 - float(decay))


def ema_step(ema, master_after, decay):
    """The EMA after one step: lerp(ema, master_after, fp32(1 - decay)) in fp32."""
    with np.errstate(all="ignore"):
        return zo.lerp32(np.ascontiguousarray(ema, F32), np.ascontiguousarray(master_after, F32),
                         weight(decay)).astype(F32)


def widen(bits):
    """uint16 bf16 codes -> float32, exactly."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def prep(g, div=1.0, coef=None):
    """The gradient the rule sees (csrc/zs_kernels.hip prep_grad without carry, before maximize):
    the sum (fp32, or bf16 codes, widened) over ``div`` in one fp32 division -- a power-of-two
    divisor's reciprocal multiply gives the same bits -- times ``coef`` in one fp32 multiply."""
    g = np.ascontiguousarray(g)
    g = widen(g) if g.dtype == np.uint16 else g.astype(F32)
    with np.errstate(all="ignore"):
        g = (g / F32(div)).astype(F32)
        if coef is not None:
            g = (g * F32(coef)).astype(F32)
    return np.ascontiguousarray(g)


def adam_ema_f32(p, g_eff, m, v, ema, hp, decay):
    """In place: fp32 parameters (their own master)."""
    c_oracle.adam_f32(p, g_eff, m, v, hp)
    ema[:] = ema_step(ema, p, decay)


def adam_ema_master(master, pb, g_eff, m, v, ema, hp, decay):
    """In place: fp32 master, bf16 parameter codes ``pb`` out."""
    c_oracle.adam_f32(master, g_eff, m, v, hp)
    pb[:] = zo.f32_to_bf16_bits(master)
    ema[:] = ema_step(ema, master, decay)


def adam_ema_split(hi, lo, g_eff, m, v, ema, hp, decay):
    """In place: the split master (hi, lo uint16); the EMA follows the stored, re-joined value."""
    p = c_oracle.join_master(hi, lo)
    c_oracle.adam_f32(p, g_eff, m, v, hp)
    hi[:], lo[:] = c_oracle.split_master(p)
    ema[:] = ema_step(ema, c_oracle.join_master(hi, lo), decay)


def same_bits(got, want, floats=True):
    """Indices where two arrays differ bit for bit; a NaN need only be a NaN (``floats``: 4-byte
    arrays are fp32, 2-byte arrays bf16 codes)."""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.itemsize == want.itemsize and got.size == want.size
    ub = np.uint32 if got.itemsize == 4 else np.uint16
    a, b = got.view(ub), want.view(ub)
    diff = a != b
    if floats:
        fa = a.view(F32) if got.itemsize == 4 else widen(a)
        fb = b.view(F32) if got.itemsize == 4 else widen(b)
        diff &= ~(np.isnan(fa) & np.isnan(fb))
    return np.flatnonzero(diff)
