"""tests/_accum_oracle.py against torch's CPU ``add_`` — what AccumulateGrad does to ``p.grad`` —
bit for bit; where the sum is a NaN both sides need only be a NaN."""
import numpy as np
import torch

import _accum_oracle as ao
import _stream_tiles as stl
from oracle import zero_oracle as zo


def _torch_add_bf16(dst_bits, src_bits):
    a = stl.as_int_tensor(dst_bits).view(torch.bfloat16).clone()
    b = stl.as_int_tensor(src_bits).view(torch.bfloat16)
    a.add_(b)
    return a.view(torch.int16).numpy().view(np.uint16)


def _torch_add_f32(dst, src):
    a = torch.from_numpy(np.ascontiguousarray(dst, np.float32).copy())
    a.add_(torch.from_numpy(np.ascontiguousarray(src, np.float32).copy()))
    return a.numpy()


def _same_bits(got, want, nan, isnan_of):
    assert np.array_equal(isnan_of(got), nan), "NaN where a number was wanted, or the reverse"
    assert np.array_equal(got[~nan], want[~nan])


def _bf16_isnan(bits):
    return np.isnan(zo.bf16_bits_to_f32(bits))


def test_every_bf16_code_against_the_eight_sources():
    dst, src = ao.bf16_table()
    assert dst.size == 8 * 65536
    want, nan = ao.add_bf16(dst, src)
    assert nan.any() and not nan.all()
    _same_bits(_torch_add_bf16(dst, src), want, nan, _bf16_isnan)
    # the tie-maker does make ties: 2^-8 is half an ulp of every code in [1, 2)
    codes = np.arange(0x3F80, 0x4000, dtype=np.uint16)
    s = zo.bf16_bits_to_f32(codes) + np.float32(2.0 ** -8)
    back = zo.bf16_bits_to_f32(zo.f32_to_bf16_bits(s))
    assert (np.abs(back - s) == np.float32(2.0 ** -8)).all()


def test_planted_bf16_cases():
    for d, s, w in ao.BF16_PLANTED:
        got, nan = ao.add_bf16(np.array([ao._b(d)], np.uint16), np.array([ao._b(s)], np.uint16))
        t = _torch_add_bf16(np.array([ao._b(d)], np.uint16), np.array([ao._b(s)], np.uint16))
        if np.isnan(w):
            assert nan[0] and _bf16_isnan(t)[0] and _bf16_isnan(got)[0]
        else:
            assert not nan[0] and got[0] == ao._b(w) == t[0], (d, s, w)
    # the cancellation gives +0, not -0
    got, _ = ao.add_bf16(np.array([ao._b(1.5)], np.uint16), np.array([ao._b(-1.5)], np.uint16))
    assert got[0] == 0x0000


def test_fp32_specials_and_random_bits():
    d, s = ao.f32_specials()
    want, nan = ao.add_f32(d, s)
    _same_bits(_torch_add_f32(d, s).view(np.uint32), want.view(np.uint32), nan,
               lambda b: np.isnan(b.view(np.float32)))
    w = want.view(np.uint32)
    assert w[0] == 0x00000002 and w[1] == 0x00800000 and w[2] == 0x007FFFFF  # denormals kept
    assert w[3] == 0x7F800000 and w[4] == 0x7F800000 and nan[5] and nan[6]
    assert w[7] == 0x00000000 and w[8] == 0x80000000 and w[9] == 0x00000000
    assert w[10] == 0x3F800000 and w[11] == 0x3F800002
    rng = np.random.default_rng(5)
    d = rng.integers(0, 2 ** 32, 1 << 18, dtype=np.uint32).view(np.float32)
    s = rng.integers(0, 2 ** 32, 1 << 18, dtype=np.uint32).view(np.float32)
    want, nan = ao.add_f32(d, s)
    _same_bits(_torch_add_f32(d, s).view(np.uint32), want.view(np.uint32), nan,
               lambda b: np.isnan(b.view(np.float32)))
    d, s = stl.wide_random(rng, 1 << 18), stl.wide_random(rng, 1 << 18)
    want, nan = ao.add_f32(d, s)
    _same_bits(_torch_add_f32(d, s).view(np.uint32), want.view(np.uint32), nan,
               lambda b: np.isnan(b.view(np.float32)))


def test_accumulate_dispatches_by_dtype():
    d = np.array([ao._b(1.0)], np.uint16)
    assert ao.accumulate(d, d)[0][0] == ao._b(2.0)
    assert ao.accumulate(np.array([1.0], np.float32), np.array([2.0], np.float32))[0][0] == 3.0
