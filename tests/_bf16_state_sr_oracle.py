"""TEST INFRASTRUCTURE — the restatement of one fused Adam step with bf16 moments stored with
stochastic rounding (``state_rounding="stochastic"``; no GPU needed, tests/test_bf16_state_sr_oracle.py
pins it).

It is tests/_bf16_state_oracle.py with ``narrow`` replaced: widen the stored bf16 ``m``, ``v``
(exact), run the unchanged fp32 oracle step — the parameter comes from the unrounded ``m'``, ``v'``
— and store them through ``sr_narrow`` with 16 bits each of ``bits(e, k0, k1)``: ``exp_avg`` the low
half, ``exp_avg_sq`` the high half.  ``e`` (uint64 array) holds every element's index in its shard's
moment array, ``keys = keys_of(seed, step)``.
"""
import numpy as np

import _accum32_oracle as a32
import _bf16_state_oracle as bo
from oracle import c_oracle
from oracle import zero_oracle as zo

widen = bo.widen
U32 = np.uint32
_M32 = np.uint64(0xFFFFFFFF)


def lowbias32(x):
    x = np.asarray(x, np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def keys_of(seed: int, t: int):
    """(k0, k1) of one launch: the optimizer's seed and the torch step of the launched part."""
    seed, t = int(seed), int(t)
    assert 0 <= seed < 1 << 64 and 0 <= t < 1 << 64
    k0 = int(lowbias32((t ^ seed) & 0xFFFFFFFF))
    k1 = int(lowbias32(((k0 ^ (seed >> 32) ^ (t >> 32)) + 0x9E3779B9) & 0xFFFFFFFF))
    return k0, k1


def bits(e, k0: int, k1: int):
    """uint32 random bits of the elements with shard indices ``e`` (uint64)."""
    e = np.asarray(e, np.uint64)
    hi = ((e >> np.uint64(32)) * np.uint64(0x9E3779B9)) & _M32
    return (lowbias32((e & _M32) ^ np.uint64(k0) ^ hi) ^ np.uint64(k1)).astype(U32)


def sr_narrow(x, r16):
    """float32 -> uint16 bf16 codes with 16 random bits ``r16`` in [0, 65535] per element: finite
    values (u + r) >> 16 with the carry kept, non-finite ones as ``zero_oracle.f32_to_bf16_bits``."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(U32).astype(np.uint64)
    r16 = np.asarray(r16).astype(np.uint64)
    assert (r16 <= 0xFFFF).all()
    out = ((u + r16) >> np.uint64(16)).astype(np.uint16)
    nonfinite = (u & np.uint64(0x7F800000)) == np.uint64(0x7F800000)
    if nonfinite.any():
        out = np.where(nonfinite, zo.f32_to_bf16_bits(x), out)
    return out


def narrow(m, v, e, keys):
    """(m bits, v bits) of the fp32 moments of the elements ``e``: one draw per element."""
    r = bits(e, *keys)
    return sr_narrow(m, r & U32(0xFFFF)), sr_narrow(v, r >> U32(16))


def _around(step, m_bits, v_bits, e, keys):
    assert m_bits.dtype == np.uint16 and v_bits.dtype == np.uint16
    assert np.shape(e) == m_bits.shape
    m, v = widen(m_bits).copy(), widen(v_bits).copy()
    step(m, v)
    m_bits[...], v_bits[...] = narrow(m, v, e, keys)


def adam_f32(p, g, m_bits, v_bits, hp, e, keys):
    """fp32 parameters, fp32 gradient."""
    _around(lambda m, v: c_oracle.adam_f32(p, g, m, v, hp), m_bits, v_bits, e, keys)


def adam_bf16(master, p_bits, g_bits, m_bits, v_bits, hp, e, keys):
    """fp32 master with its bf16 copy ``p_bits``, bf16 gradient."""
    _around(lambda m, v: c_oracle.adam_bf16(master, p_bits, g_bits, m, v, hp), m_bits, v_bits, e, keys)


def adam_bf16_split(hi, lo, g_bits, m_bits, v_bits, hp, e, keys):
    """Split master, bf16 gradient."""
    _around(lambda m, v: c_oracle.adam_bf16_split(hi, lo, g_bits, m, v, hp), m_bits, v_bits, e, keys)


def adam_f32grad_split(hi, lo, g, m_bits, v_bits, hp, e, keys):
    """Split master, fp32 gradient (ZeRO-3's fp32 accumulation arena)."""
    _around(lambda m, v: a32.adam_f32grad_split(hi, lo, g, m, v, hp), m_bits, v_bits, e, keys)


def decay(code_bits, beta, steps, seed=0):
    """``steps`` pure decays x <- sr(beta * x) of the bf16 values ``code_bits`` (one fp32 multiply,
    element i at shard index i, step t keyed as the optimizer keys it, the exp_avg_sq half of the
    draw): what the update does to exp_avg_sq at a zero gradient."""
    x = np.ascontiguousarray(code_bits, np.uint16).copy()
    e = np.arange(x.size, dtype=np.uint64)
    for t in range(1, steps + 1):
        r = bits(e, *keys_of(seed, t))
        with np.errstate(all="ignore"):
            x = sr_narrow((widen(x) * np.float32(beta)).astype(np.float32), r >> U32(16))
    return x
