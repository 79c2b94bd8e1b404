"""TEST INFRASTRUCTURE — the restatement of one master-free fused Adam step (``master="none"``,
p_dtype ZS_BF16_SR; no GPU needed, tests/test_psr_oracle.py pins it).

It composes pieces that exist and writes no arithmetic of its own: widen the stored bf16 parameter,
the gradient and the moments (exact), run the unchanged fp32 oracle step ``c_oracle.adam_f32``,
store the moments as their state says — fp32 as they are, ``_bf16_state_oracle.narrow`` (nearest) or
``_bf16_state_sr_oracle.narrow`` (stochastic, the draws of ``bits(e, k0, k1)``) — and the parameter
as ``sr_narrow(p', bits(e, *pkeys(k0, k1)) & 0xFFFF)``.  ``e`` (uint64 array) holds every element's
index in its shard's moment array, ``keys = keys_of(seed, step)``.
"""
import numpy as np

import _bf16_state_oracle as bo
import _bf16_state_sr_oracle as so
from oracle import c_oracle

STATES = ("f32", "bf16", "bf16_sr")  # fp32 moments; bf16 to nearest; bf16 stochastically
widen, keys_of, bits, sr_narrow, lowbias32 = bo.widen, so.keys_of, so.bits, so.sr_narrow, so.lowbias32


def pkeys(k0: int, k1: int):
    """(kp0, kp1): the keys of the parameter's draw, from the launch's keys."""
    kp0 = int(lowbias32((int(k0) ^ 0x85EBCA6B) & 0xFFFFFFFF))
    kp1 = int(lowbias32((int(k1) + 0xC2B2AE35) & 0xFFFFFFFF))
    return kp0, kp1


def r16p(e, keys):
    """The 16 bits the parameters of the elements ``e`` round with."""
    return bits(e, *pkeys(*keys)) & np.uint32(0xFFFF)


def narrow_param(p, e, keys):
    """float32 parameters of the elements ``e`` -> the bf16 codes they are stored as."""
    return sr_narrow(p, r16p(e, keys))


def step(p_bits, g, m, v, hp, e, keys, state):
    """In place: bf16 parameters ``p_bits`` (uint16), moments ``m`` / ``v`` (float32 for state
    "f32", uint16 otherwise) after one step with the gradient ``g`` (uint16 bf16 codes, or float32:
    the fp32-gradient form)."""
    assert state in STATES and p_bits.dtype == np.uint16 and np.shape(e) == p_bits.shape
    p = widen(p_bits).copy()
    gf = np.ascontiguousarray(g if g.dtype == np.float32 else widen(g))
    if state == "f32":
        assert m.dtype == np.float32 and v.dtype == np.float32
        mm, vv = np.ascontiguousarray(m), np.ascontiguousarray(v)
    else:
        assert m.dtype == np.uint16 and v.dtype == np.uint16
        mm, vv = widen(m).copy(), widen(v).copy()
    c_oracle.adam_f32(p, gf, mm, vv, hp)
    if state == "f32":
        m[...], v[...] = mm, vv
    elif state == "bf16":
        m[...], v[...] = bo.narrow(mm), bo.narrow(vv)
    else:
        m[...], v[...] = so.narrow(mm, vv, e, keys)
    p_bits[...] = narrow_param(p, e, keys)
