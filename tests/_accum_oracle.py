"""numpy restatement of zs_accumulate (dst[i] = dst[i] + src[i]) and the value tables its tests
share (no GPU needed; tests/test_accum_oracle.py pins it against torch's CPU ``add_``).

fp32: one ``np.float32`` add.  bf16 (uint16 bit patterns): both operands widened exactly, one fp32
add, one round-to-nearest-even to bf16 — ``oracle.zero_oracle``'s conversions.
"""
import numpy as np

from oracle import zero_oracle as zo

assert np.float32(2.0 ** -149) + np.float32(2.0 ** -149) == 2.0 ** -148, "numpy flushed a denormal"


def add_f32(dst, src):
    """(dst + src in fp32, mask of the sums that are NaN)."""
    with np.errstate(all="ignore"):
        s = np.asarray(dst, np.float32) + np.asarray(src, np.float32)
    assert s.dtype == np.float32
    return s, np.isnan(s)


def add_bf16(dst_bits, src_bits):
    """(bf16 bits of RNE(widened dst + widened src), mask of the sums that are NaN)."""
    s, nan = add_f32(zo.bf16_bits_to_f32(np.asarray(dst_bits, np.uint16)),
                     zo.bf16_bits_to_f32(np.asarray(src_bits, np.uint16)))
    return zo.f32_to_bf16_bits(s), nan


def accumulate(dst, src):
    """By dtype: float32 arrays, or uint16 arrays of bf16 bit patterns."""
    return add_bf16(dst, src) if np.asarray(dst).dtype == np.uint16 else add_f32(dst, src)


# ---- value tables ----------------------------------------------------------------------------
# the eight bf16 sources every bf16 code is added to: +0, -0, 2^-8 (makes ties of the codes with
# exponent 0: half an ulp of [1, 2)), +max, -max, +inf, a NaN, the smallest denormal
BF16_SOURCES = np.array([0x0000, 0x8000, 0x3B80, 0x7F7F, 0xFF7F, 0x7F80, 0x7FC0, 0x0001], np.uint16)
assert zo.bf16_bits_to_f32(BF16_SOURCES[2:3])[0] == np.float32(2.0 ** -8)

ALL_BF16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def bf16_table():
    """(dst bits, src bits): every bf16 code against each of the eight sources, 8 x 65,536."""
    dst = np.tile(ALL_BF16, len(BF16_SOURCES))
    src = np.repeat(BF16_SOURCES, ALL_BF16.size)
    return dst, src


def _b(x):
    return zo.f32_to_bf16_bits(np.asarray([x], np.float32))[0]


# planted bf16 cases (dst, src, want) as values exactly representable in bf16
BF16_PLANTED = [
    (1.0, 2.0 ** -8, 1.0),                          # tie, rounds down to the even code
    (1.0 + 2.0 ** -7, 2.0 ** -8, 1.0 + 2.0 ** -6),  # tie, rounds up to the even code
    (3.3895314e38, 3.3895314e38, np.inf),           # overflow
    (np.inf, -np.inf, np.nan),
    (1.5, -1.5, 0.0),                               # cancellation: +0
]

# fp32 specials: (dst bits, src bits) as uint32
F32_SPECIALS = np.array([
    (0x00000001, 0x00000001),  # denormal + denormal
    (0x007FFFFF, 0x00000001),  # largest denormal + smallest: FLT_MIN
    (0x00800000, 0x80000001),  # FLT_MIN - denormal: back into the denormals
    (0x7F7FFFFF, 0x7F7FFFFF),  # overflow to inf
    (0x7F7FFFFF, 0x73000000),  # FLT_MAX + half an ulp: tie, rounds to inf
    (0x7F800000, 0xFF800000),  # inf - inf: NaN
    (0x7FC00000, 0x3F800000),  # NaN + 1
    (0x3F800000, 0xBF800000),  # cancellation: +0
    (0x80000000, 0x80000000),  # -0 + -0 = -0
    (0x80000000, 0x00000000),  # -0 + +0 = +0
    (0x3F800000, 0x33800000),  # 1 + 2^-24: tie, rounds down
    (0x3F800001, 0x33800000),  # (1 + 2^-23) + 2^-24: tie, rounds up
    (0x4B800000, 0x3F800000),  # 2^24 + 1: tie
    (0xFF7FFFFF, 0xFF7FFFFF),  # -overflow
], np.uint32)


def f32_specials():
    return F32_SPECIALS[:, 0].copy().view(np.float32), F32_SPECIALS[:, 1].copy().view(np.float32)
