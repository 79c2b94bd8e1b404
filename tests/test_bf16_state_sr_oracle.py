"""Stochastic rounding of bf16 Adam moments, on the CPU: the rounding and the generator of
tests/_bf16_state_sr_oracle.py against ``zero_oracle.f32_to_bf16_bits``, against the library's host
functions (zs_sr_keys / zs_sr_bits through ctypes) and against their own statistics, and the guard
that lets torch's default betas through only under stochastic rounding.
"""
import ctypes

import numpy as np
import pytest

import _bf16_state_oracle as bo
import _bf16_state_sr_oracle as so
from _stream_tiles import SPECIALS_NO_NAN, wide_random
from oracle import zero_oracle as zo
from test_bf16_state_oracle import _normal_bf16

U32 = np.uint32


def _rne_r(x):
    """The r under which the stochastic formula is round-to-nearest-even: 0x7FFF + lsb(hi)."""
    u = np.ascontiguousarray(x, np.float32).view(U32)
    return U32(0x7FFF) + ((u >> U32(16)) & U32(1))


def test_identity_with_round_to_nearest_even():
    x = np.concatenate([SPECIALS_NO_NAN, wide_random(np.random.default_rng(3), 1 << 18)])
    assert np.isinf(x).any() and (np.abs(x[np.isfinite(x)]) < 1e-38).any()
    assert np.array_equal(so.sr_narrow(x, _rne_r(x)), zo.f32_to_bf16_bits(x))


def test_non_finite_inputs_ignore_r():
    x = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF,
                  0xFFC12345], U32).view(np.float32)
    want = zo.f32_to_bf16_bits(x)
    assert (want[2:] & 0x7FFF > 0x7F80).all()  # a NaN stays a NaN
    for r in (0, 1, 0x7FFF, 0x8000, 0xFFFF):
        assert np.array_equal(so.sr_narrow(x, np.full(x.size, r, U32)), want), r


@pytest.mark.parametrize("hi", [0x3F80, 0x0000, 0x8001, 0x7F7E, 0xC2F7, 0x0080])
def test_round_up_count_is_the_low_half(hi):
    """For a fixed high half and every low half L, exactly L of the 65,536 values of r round away
    from zero (so the probability is L / 65536 and the rounding is unbiased).  The full product is
    2^32 roundings per high half, so: counted over every r for 258 low halves (every 257th, and
    both ends), where the code is also seen to take the two neighbours only and never to fall as r
    grows; and for every L the last r that stays (65535 - L) and the first that leaves (65536 - L),
    which with that monotonicity is the count."""
    r = np.arange(65536, dtype=U32)
    word = lambda lows: ((U32(hi) << U32(16)) | np.asarray(lows, U32)).view(np.float32)  # noqa: E731
    for L in sorted(set(range(0, 65536, 257)) | {1, 65535}):
        got = so.sr_narrow(np.repeat(word([L]), 65536), r)
        assert ((got == hi) | (got == hi + 1)).all() and (np.diff(got.astype(np.int64)) >= 0).all()
        assert int((got != hi).sum()) == L, L
    lows = np.arange(65536, dtype=U32)
    assert (so.sr_narrow(word(lows), U32(65535) - lows) == hi).all()
    assert (so.sr_narrow(word(lows[1:]), U32(65536) - lows[1:]) == hi + 1).all()
    assert (so.sr_narrow(word(lows), np.zeros(65536, U32)) == hi).all()
    assert (so.sr_narrow(word(lows[1:]), np.full(65535, 65535, U32)) == hi + 1).all()


def test_carry_out_of_the_largest_finite_value_is_inf():
    x = np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0001, 0xFF7F0001, 0x7F7F0000], U32).view(np.float32)
    got = so.sr_narrow(x, np.array([1, 1, 0xFFFF, 0xFFFF, 0xFFFF], U32))
    assert got.tolist() == [0x7F80, 0xFF80, 0x7F80, 0xFF80, 0x7F7F]


SEEDS = (0, (1 << 32) + 12345, 0xDEADBEEFCAFEF00D)
STEPS = (1, 2, (1 << 32) + 1)
INDICES = [0, 1, 2, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) - 1, 1 << 40,
           (1 << 40) + 7]


def test_host_functions_equal_numpy():
    from zero_amd import _lib

    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    P32 = ctypes.POINTER(ctypes.c_uint32)
    raw.zs_sr_keys.argtypes = [ctypes.c_uint64, ctypes.c_uint64, P32, P32]
    raw.zs_sr_bits.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, P32]
    for seed in SEEDS:
        for t in STEPS:
            k0, k1, r = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
            assert raw.zs_sr_keys(seed, t, ctypes.byref(k0), ctypes.byref(k1)) == _lib.ZS_OK
            assert (k0.value, k1.value) == so.keys_of(seed, t), (seed, t)
            want = so.bits(np.array(INDICES, np.uint64), k0.value, k1.value)
            for e, w in zip(INDICES, want):
                assert raw.zs_sr_bits(e, k0.value, k1.value, ctypes.byref(r)) == _lib.ZS_OK
                assert r.value == int(w), (seed, t, e)
    assert raw.zs_sr_keys(0, 1, None, None) == _lib.ZS_ERR_INVALID
    assert raw.zs_sr_bits(0, 0, 0, None) == _lib.ZS_ERR_INVALID


def test_wrappers_equal_numpy():
    from zero_amd.kernels import sr_bits, sr_keys

    keys = sr_keys(SEEDS[1], 7)
    assert keys == so.keys_of(SEEDS[1], 7)
    assert sr_bits(INDICES[5], keys) == int(so.bits(np.array([INDICES[5]], np.uint64), *keys)[0])


def test_generator_statistics():
    """Uniform halves, uncorrelated halves and steps, one rounding unbiased: bounds of six standard
    errors of the statistic over N = 2^20 draws (a uniform 16-bit field has standard deviation
    65535 / sqrt(12); a correlation coefficient of independent draws 1 / sqrt(N))."""
    n = 1 << 20
    e = np.arange(n, dtype=np.uint64) + np.uint64(1)
    r1, r2 = so.bits(e, *so.keys_of(0, 1)), so.bits(e, *so.keys_of(0, 2))
    lo, hi = (r1 & U32(0xFFFF)).astype(np.float64), (r1 >> U32(16)).astype(np.float64)
    se_mean = (1 / np.sqrt(12)) / np.sqrt(n)
    for name, h in (("low", lo), ("high", hi)):
        mean = h.mean() / 65535
        print(f"{name} half: mean {mean:.5f}")
        assert abs(mean - 0.5) <= 6 * se_mean
    c_halves = np.corrcoef(lo, hi)[0, 1]
    c_steps = np.corrcoef(hi, (r2 >> U32(16)).astype(np.float64))[0, 1]
    print(f"correlation of the halves {c_halves:.1e}, of consecutive steps {c_steps:.1e}")
    assert abs(c_halves) <= 6 / np.sqrt(n) and abs(c_steps) <= 6 / np.sqrt(n)
    # no index draws the same bits at every step (element 0 included)
    for e0 in (0, 1, 1 << 32):
        draws = {int(so.bits(np.array([e0], np.uint64), *so.keys_of(0, t))[0]) for t in range(1, 65)}
        assert len(draws) == 64, e0
    # one rounding of values with uniform low halves: the error in bf16 ulps has mean 0 and
    # standard deviation below 1/2
    x = (U32(0x3F800000) | (so.bits(e, 11, 12) & U32(0x007FFFFF))).view(np.float32)
    got = so.sr_narrow(x, r1 >> U32(16))
    err = (got.astype(np.int64) << 16) - x.view(U32).astype(np.int64)
    bias = err.mean() / 65536
    print(f"bias of one rounding {bias:.1e} bf16 ulp")
    assert abs(bias) <= 6 * 0.5 / np.sqrt(n)


def test_decay_at_torchs_default_beta2():
    """20,000 bf16 values spanning the normal range under x <- sr(0.999 * x) for 1000 steps: every
    value moved, and the mean ratio to 0.999^1000 is 1 within 5 standard errors of the sample.
    (Rounded to nearest none of them moves: tests/test_bf16_state_oracle.py.)"""
    code = _normal_bf16()
    assert len(code) == 20000
    x0 = bo.widen(code).astype(np.float64)
    assert np.log10(x0.max() / x0.min()) > 16
    beta, steps = 0.999, 1000
    after = so.decay(code, beta, steps)
    assert (after != code).all()
    x1 = bo.widen(after).astype(np.float64)
    # values that decayed into the denormals lose bits: their ratio is taken as it is
    ratio = x1 / x0 / float(np.float32(beta)) ** steps
    mean, se = ratio.mean(), ratio.std() / np.sqrt(ratio.size)
    print(f"mean ratio {mean:.5f}, standard error {se:.1e}, {abs(mean - 1) / se:.2f} standard "
          f"errors, spread {ratio.std():.3f}")
    assert abs(mean - 1) <= 5 * se


def test_guard_under_both_roundings():
    from zero_amd._update import check_bf16_state_group, check_state_rounding
    import torch

    default = dict(beta1=0.9, beta2=0.999, amsgrad=False)
    check_bf16_state_group(default, "stochastic")
    check_bf16_state_group(dict(beta1=0.9999, beta2=0.99999, amsgrad=False), "stochastic")
    for rounding in (None, "nearest"):
        with pytest.raises(ValueError, match=r"beta2.*0\.99609375"):
            check_bf16_state_group(default, rounding)
    with pytest.raises(ValueError, match=r"beta2.*0\.99609375"):
        check_bf16_state_group(default)
    for rounding in (None, "nearest", "stochastic"):
        with pytest.raises(ValueError, match="amsgrad"):
            check_bf16_state_group({**default, "beta2": 0.95, "amsgrad": True}, rounding)
    BF16 = torch.bfloat16
    assert check_state_rounding(None, 0, torch.float32) == ("nearest", 0)
    assert check_state_rounding("nearest", 5, BF16) == ("nearest", 5)
    assert check_state_rounding("stochastic", (1 << 64) - 1, BF16) == ("stochastic", (1 << 64) - 1)
    with pytest.raises(ValueError, match="state_dtype=torch.bfloat16"):
        check_state_rounding("stochastic", 0, torch.float32)
    for bad in ("random", "", 1, True):
        with pytest.raises(ValueError, match="state_rounding"):
            check_state_rounding(bad, 0, BF16)
    for bad in (-1, 1 << 64, 1.5, "7", None, True):
        with pytest.raises(ValueError, match="state_seed"):
            check_state_rounding("stochastic", bad, BF16)


def test_checkpoint_header_carries_the_seed():
    from zero_amd import checkpoint as ckpt

    h = ckpt.header(2, 1, 0, [0, 1])
    assert "state_seed" not in h and ckpt.saved_state_seed({"zero_amd": h}) is None
    h = ckpt.header(2, 1, 0, [0, 1], state_seed=(1 << 63) + 5)
    assert ckpt.saved_state_seed({"zero_amd": h}) == (1 << 63) + 5
    ckpt.check_header({"zero_amd": h}, ckpt.header(2, 1, 0, [0, 1], state_seed=9))  # not compared
    ckpt.check_header({"zero_amd": h}, ckpt.header(2, 1, 0, [0, 1]))
    assert ckpt.saved_state_seed({}) is None
