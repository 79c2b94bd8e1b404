"""TEST INFRASTRUCTURE — numpy statement of the row-scaled fp8 (OCP E4M3) gather kernels' contract.

The format is stated from its bit fields (1 sign, 4 exponent bits with bias 7, 3 mantissa bits; no
infinities; S.1111.111 is NaN, so the largest finite value is S.1111.110 = 448), the rounding as
"nearest representable value, ties to the even code", in float64.  Only the steps that the kernels
define as fp32 operations (amax, inv = 448 / a, scale = a / 448, the product x * inv, and the one
rounding of decode * scale) are fp32 here.  No torch: tests/test_fp8_oracle.py pins encode and
decode against torch's float8_e4m3fn on every code, every bf16 value of |x| <= 448 and every
rounding midpoint.

The contract ("fp8 rows: the contract"), per row:
  amax  = fp32 max of |x| over the row's non-NaN elements
  amax == 0:  inv = scale = 1
  otherwise:  a = max(amax, 2^-116), inv = 448 / a, scale = a / 448
  q     = e4m3(RNE(x * inv)) (|x * inv| <= 448 * (1 + 2^-23), which rounds to 448); an element
          whose product is NaN (a NaN element, or ±Inf times the inv = 0 of a row that holds an
          Inf) is stored as the NaN code 0xFF, whatever its sign: what the gfx950 conversion
          instruction makes of a NaN
  deq   = float32(decode(q) * scale), then RNE to bf16 for bf16 output
"""
from __future__ import annotations

import numpy as np

E4M3_MAX = 448.0
AMAX_FLOOR = np.float32(2.0 ** -116)
NAN_CODE = 0x7F
ROW_NAN_CODE = 0xFF  # quantize_rows' code of a NaN product


def e4m3_decode(codes) -> np.ndarray:
    """uint8 codes -> float64 values, from the bit fields; 0x7F and 0xFF decode to NaN."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    sign = np.where(c & 0x80, -1.0, 1.0)
    e = (c >> 3) & 0xF
    m = (c & 0x7).astype(np.float64)
    mag = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * np.exp2((e - 7).astype(np.float64)))
    mag = np.where((c & 0x7F) == NAN_CODE, np.nan, mag)
    return np.copysign(mag, sign)


# the 127 non-negative finite values, in code order (which is value order)
_FINITE = e4m3_decode(np.arange(NAN_CODE, dtype=np.uint8))


def e4m3_encode(x) -> np.ndarray:
    """float32 values -> uint8 codes: nearest representable value, ties to the even code,
    saturating at ±448 (±Inf included); NaN -> 0x7F | sign."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    sign = ((x.view(np.uint32) >> np.uint32(24)) & np.uint32(0x80)).astype(np.uint8)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):  # (a signalling NaN's widening cast)
        a = np.where(nan, 0.0, np.minimum(np.abs(x.astype(np.float64)), E4M3_MAX))
    hi = np.minimum(np.searchsorted(_FINITE, a, side="left"), NAN_CODE - 1)  # first value >= a
    lo = np.maximum(hi - 1, 0)
    d_lo, d_hi = a - _FINITE[lo], _FINITE[hi] - a  # exact: float64 holds every difference
    code = np.where(d_lo < d_hi, lo, np.where(d_hi < d_lo, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(nan, NAN_CODE, code).astype(np.uint8)
    return code | sign


def f32_to_bf16_bits(x) -> np.ndarray:
    """float32 -> bf16 bit patterns (uint16), round to nearest even; NaN stays NaN (quieted)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(x), ((u >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def bf16_bits_to_f32(h) -> np.ndarray:
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def row_scales(x):
    """(amax, inv, scale), float32 each, of the rows of a 2-D float32 array."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2
    amax = np.fmax.reduce(np.abs(x), axis=1, initial=np.float32(0)).astype(np.float32)  # fmax: NaN dropped
    a = np.maximum(amax, AMAX_FLOOR)
    with np.errstate(all="ignore"):
        inv = np.where(amax > 0, np.float32(E4M3_MAX) / a, np.float32(1)).astype(np.float32)
        scale = np.where(amax > 0, a / np.float32(E4M3_MAX), np.float32(1)).astype(np.float32)
    return amax, inv, scale


def quantize_rows(x):
    """(q uint8, scales float32) of a 2-D array of float32 values (a bf16 input is passed as the
    float32 values it holds)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    _, inv, scale = row_scales(x)
    with np.errstate(all="ignore"):
        p = (x * inv[:, None]).astype(np.float32)  # the kernel's fp32 product
    q = np.where(np.isnan(p), np.uint8(ROW_NAN_CODE), e4m3_encode(p)).astype(np.uint8)
    return q, scale


def dequantize_rows(q, scales, dtype="float32"):
    """decode(q) * scale per row, rounded ONCE from the exact float64 product to float32
    (dtype "float32": returns float32), then RNE to bf16 (dtype "bfloat16": returns the uint16
    bit patterns).  NaN codes, 0 * Inf and the like give NaN."""
    q = np.asarray(q, dtype=np.uint8)
    assert q.ndim == 2 and str(dtype) in ("float32", "bfloat16")
    with np.errstate(all="ignore"):
        # a 4-bit significand times a 24-bit one: the float64 product is exact
        y = (e4m3_decode(q) * np.asarray(scales, dtype=np.float32).astype(np.float64)[:, None]).astype(np.float32)
    return y if str(dtype) == "float32" else f32_to_bf16_bits(y)
