"""numpy restatement of zs_accumulate_widen and of the fp32-gradient split-master updates (no GPU
needed; tests/test_accum32_oracle.py pins them against torch's CPU arithmetic and the C oracle).

Widen-add: a bf16 code becomes the fp32 value with those 16 bits on top (a bit-field move, exact),
then one ``np.float32`` add.  The updates are composed from the existing oracles, which are not
touched: join the split master to fp32, run the fp32 update on it, split the result again.
"""
import numpy as np

import _sgd_oracle as so
from oracle import c_oracle

assert np.float32(2.0 ** -149) + np.float32(2.0 ** -149) == 2.0 ** -148, "numpy flushed a denormal"


def widen(bits):
    """uint16 bf16 codes -> float32, exactly."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def widen_first(a_bits, src_bits):
    """zs_accumulate_widen with a != NULL: widen(a) + widen(src), one fp32 add."""
    with np.errstate(all="ignore"):
        out = widen(a_bits) + widen(src_bits)
    assert out.dtype == np.float32
    return out


def widen_add(dst, src_bits):
    """zs_accumulate_widen with a == NULL: dst + widen(src), one fp32 add."""
    dst = np.ascontiguousarray(dst)
    assert dst.dtype == np.float32
    with np.errstate(all="ignore"):
        out = dst + widen(src_bits)
    assert out.dtype == np.float32
    return out


def accumulate_passes(chunks):
    """The arena after the passes delivered ``chunks`` (uint16 arrays, pass order): bf16 bits after
    one pass, the fp32 sum (widen_first, then widen_add per further pass) after more."""
    if len(chunks) == 1:
        return np.ascontiguousarray(chunks[0], np.uint16)
    acc = widen_first(chunks[0], chunks[1])
    for c in chunks[2:]:
        acc = widen_add(acc, c)
    return acc


def adam_f32grad_split(hi, lo, g, m, v, hp, vmax=None):
    """In place: the split master (hi, lo uint16) updated with an fp32 gradient."""
    p = c_oracle.join_master(hi, lo)
    c_oracle.adam_f32(p, np.ascontiguousarray(g, np.float32), m, v, hp, vmax=vmax)
    hi[:], lo[:] = c_oracle.split_master(p)


def sgd_f32grad_split(hi, lo, g, buf, hp, coef=None):
    """(hi, lo, buf) after one SGD step of the split master with an fp32 gradient."""
    p, buf, _ = so.step_f32(c_oracle.join_master(hi, lo), np.ascontiguousarray(g, np.float32), buf,
                            hp, coef=coef)
    hi, lo = c_oracle.split_master(p)
    return hi, lo, buf


# ---- the planted sequence of the issue: 1.0, then 2^-9 seven times -----------------------------
PLANTED = [1.0] + [2.0 ** -9] * 7


def planted_bits():
    return [so.f32_to_bf16_bits(np.array([x], np.float32)) for x in PLANTED]


def fp32_bound(chunks):
    """(N - 1) * 2^-24 * sum_k |g_k| per element, in float64."""
    mag = sum(np.abs(widen(c).astype(np.float64)) for c in chunks)
    return (len(chunks) - 1) * 2.0 ** -24 * mag


def exact_sum(chunks):
    return sum(widen(c).astype(np.float64) for c in chunks)
