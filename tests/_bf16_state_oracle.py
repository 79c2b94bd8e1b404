"""TEST INFRASTRUCTURE — the restatement of one fused Adam step with bf16 moments
(``state_dtype=torch.bfloat16``), composed from oracles that are not touched (no GPU needed;
tests/test_bf16_state_oracle.py pins it against the numpy restatement).

One step: widen the stored bf16 ``m``, ``v`` to fp32 (a bit-field move, exact), run the existing
fp32 step on them — the parameter therefore comes from the unrounded fp32 ``m'``, ``v'`` — and store
``m'``, ``v'`` rounded to nearest even (``zero_oracle.f32_to_bf16_bits``: a NaN stays a NaN, what
lies past the largest bf16 becomes Inf).  ``m_bits`` / ``v_bits`` are uint16 arrays, updated in place
like every other array the C oracle takes.
"""
import numpy as np

import _accum32_oracle as a32
from oracle import c_oracle
from oracle import zero_oracle as zo

MIN_ONE_MINUS_BETA = 2.0 ** -8  # the guard: below it a bf16 value no longer moves under the decay


def widen(bits):
    """uint16 bf16 codes -> float32, exactly."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow(x):
    """float32 -> uint16 bf16 codes, round to nearest even."""
    return zo.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32))


def _around(step, m_bits, v_bits):
    assert m_bits.dtype == np.uint16 and v_bits.dtype == np.uint16
    m, v = widen(m_bits).copy(), widen(v_bits).copy()
    step(m, v)
    m_bits[...], v_bits[...] = narrow(m), narrow(v)


def adam_f32(p, g, m_bits, v_bits, hp):
    """fp32 parameters, fp32 gradient."""
    _around(lambda m, v: c_oracle.adam_f32(p, g, m, v, hp), m_bits, v_bits)


def adam_bf16(master, p_bits, g_bits, m_bits, v_bits, hp):
    """fp32 master with its bf16 copy ``p_bits``, bf16 gradient."""
    _around(lambda m, v: c_oracle.adam_bf16(master, p_bits, g_bits, m, v, hp), m_bits, v_bits)


def adam_bf16_split(hi, lo, g_bits, m_bits, v_bits, hp):
    """Split master, bf16 gradient."""
    _around(lambda m, v: c_oracle.adam_bf16_split(hi, lo, g_bits, m, v, hp), m_bits, v_bits)


def adam_f32grad_split(hi, lo, g, m_bits, v_bits, hp):
    """Split master, fp32 gradient (ZeRO-3's fp32 accumulation arena)."""
    _around(lambda m, v: a32.adam_f32grad_split(hi, lo, g, m, v, hp), m_bits, v_bits)


def numpy_step(p, g, m_bits, v_bits, step, **kw):
    """The same composition over ``zero_oracle.adam_update``: (p', m' bits, v' bits)."""
    p, m, v, _ = zo.adam_update(p, g, widen(m_bits), widen(v_bits), step, **kw)[:4]
    return p, narrow(m), narrow(v)


def decays(bits, beta):
    """Which of the bf16 values ``bits`` change under one pure decay x <- bf16(beta * x), the
    product one fp32 multiply (what the update does to exp_avg_sq at a zero gradient)."""
    with np.errstate(all="ignore"):
        after = narrow((widen(bits) * np.float32(beta)).astype(np.float32))
    return after != np.asarray(bits, np.uint16)
