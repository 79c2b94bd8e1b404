"""tests/_accum32_oracle.py against torch's CPU arithmetic and the C oracle, bit for bit (where a
sum is a NaN both sides need only be a NaN), and the error bounds DESIGN.md states for fp32 and
bf16 accumulation on the planted sequence 1.0, then 2^-9 seven times."""
import numpy as np
import pytest
import torch

import _accum32_oracle as a32
import _accum_oracle as ao
import _sgd_oracle as so
import _stream_tiles as stl
from oracle import c_oracle


def _bf16_tensor(bits):
    return stl.as_int_tensor(np.ascontiguousarray(bits, np.uint16)).view(torch.bfloat16)


def _same(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN where a number was wanted, or the reverse"
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    return nan


def test_widen_is_the_bit_field_move():
    w = a32.widen(ao.ALL_BF16)
    assert np.array_equal(w.view(np.uint32), ao.ALL_BF16.astype(np.uint32) << 16)
    t = _bf16_tensor(ao.ALL_BF16).float().numpy()
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(t), nan)
    assert np.array_equal(t.view(np.uint32)[~nan], w.view(np.uint32)[~nan])


def test_first_mode_every_bf16_code_against_the_eight_sources():
    a, src = ao.bf16_table()
    assert a.size == 8 * 65536
    want = _bf16_tensor(a).float() + _bf16_tensor(src).float()
    nan = _same(a32.widen_first(a, src), want.numpy())
    assert nan.any() and not nan.all()


def test_second_mode_every_bf16_code_and_the_fp32_specials():
    # dst = the widened codes plus one earlier contribution (so it is no longer bf16-representable)
    a, src = ao.bf16_table()
    dst = a32.widen_first(a, np.full(a.size, 0x3B80, np.uint16))  # + 2^-8
    acc = torch.from_numpy(dst.copy())
    acc.add_(_bf16_tensor(src).float())
    _same(a32.widen_add(dst, src), acc.numpy())
    # every fp32 special against every source
    d = np.repeat(np.concatenate([ao.F32_SPECIALS[:, 0], ao.F32_SPECIALS[:, 1]]).view(np.float32),
                  ao.BF16_SOURCES.size)
    s = np.tile(ao.BF16_SOURCES, d.size // ao.BF16_SOURCES.size)
    acc = torch.from_numpy(d.copy())
    acc.add_(_bf16_tensor(s).float())
    got = a32.widen_add(d, s)
    _same(got, acc.numpy())
    one = np.array([0x0001], np.uint16)  # the smallest bf16 denormal, 2^-133: kept, not flushed
    assert a32.widen_add(np.zeros(1, np.float32), one).view(np.uint32)[0] == 0x00010000
    assert a32.widen_first(one, one).view(np.uint32)[0] == 0x00020000
    inf, ninf = np.array([0x7F80], np.uint16), np.array([0xFF80], np.uint16)
    assert np.isnan(a32.widen_first(inf, ninf)[0])
    assert np.isnan(a32.widen_add(np.array([np.inf], np.float32), ninf)[0])
    mz = np.array([0x8000], np.uint16)
    assert a32.widen_first(mz, mz).view(np.uint32)[0] == 0x80000000
    assert a32.widen_first(mz, np.zeros(1, np.uint16)).view(np.uint32)[0] == 0


def _masters(rng, n):
    """Random masters with planted split-master ties (low half 0x8000: stored 1 ulp toward zero)
    and near-ties."""
    u = (rng.standard_normal(n).astype(np.float32) * np.float32(0.3)).view(np.uint32).copy()
    u[::7] = (u[::7] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    u[1::11] = (u[1::11] & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)
    u[2::13] = (u[2::13] & np.uint32(0xFFFF0000)) | np.uint32(0x8001)
    return c_oracle.split_master(u.view(np.float32))


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("wd,decoupled,maximize", [(0.0, False, False), (0.01, False, False),
                                                   (0.01, True, False), (0.0, False, True),
                                                   (0.1, True, True)])
def test_composed_adam_equals_the_split_oracle_on_bf16_gradients(amsgrad, wd, decoupled, maximize):
    rng = np.random.default_rng(11)
    n = 4096 + 257
    hi, lo = _masters(rng, n)
    # a tie rounds to the even code: down (stored as 0x7FFF) or up (residual -0x8000)
    assert (lo == 0x7FFF).sum() >= n // 14 and (lo == 0x8000).sum() >= n // 28
    g_bits = so.f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32) * np.float32(0.05))
    g_bits[::5] = 0  # no gradient: the master's ties must survive the round trip
    st = [[hi.copy(), lo.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32),
           np.zeros(n, np.float32) if amsgrad else None] for _ in range(2)]
    for step in (1, 2, 3):
        # lr = 0 on the second step: the update leaves every master, ties included, where it is
        hp = c_oracle.hparams(lr=0.0 if step == 2 else 1e-2, weight_decay=wd, step=step,
                              decoupled=decoupled, amsgrad=amsgrad, maximize=maximize, grad_div=2.0)
        a, b = st
        c_oracle.adam_bf16_split(a[0], a[1], g_bits, a[2], a[3], hp, vmax=a[4])
        a32.adam_f32grad_split(b[0], b[1], a32.widen(g_bits), b[2], b[3], hp, vmax=b[4])
        for x, y in zip(a, b):
            if x is not None:
                assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else np.uint16),
                                      y.view(np.uint32 if y.dtype == np.float32 else np.uint16)), step


@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
def test_composed_sgd_equals_the_split_oracle_on_bf16_gradients(momentum, nesterov):
    rng = np.random.default_rng(12)
    n = 1024 + 61
    hi, lo = _masters(rng, n)
    g_bits = so.f32_to_bf16_bits(rng.standard_normal(n).astype(np.float32) * np.float32(0.05))
    a = (hi.copy(), lo.copy(), None)
    b = (hi.copy(), lo.copy(), None)
    for step in (1, 2, 3):
        hp = so.SgdHP(0.05, momentum, weight_decay=0.01, nesterov=nesterov, first=step == 1,
                      grad_div=3.0)
        ah, al, ab, _ = so.step_split(a[0], a[1], g_bits, a[2], hp)
        a = (ah, al, ab)
        b = a32.sgd_f32grad_split(b[0], b[1], a32.widen(g_bits), b[2], hp)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        if momentum:
            assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def test_planted_sequence_breaks_the_fp32_bound_in_bf16_and_meets_it_in_fp32():
    chunks = a32.planted_bits()
    assert [float(a32.widen(c)[0]) for c in chunks] == a32.PLANTED
    exact = a32.exact_sum(chunks)[0]
    assert exact == 1.0 + 7 * 2.0 ** -9
    n = len(chunks)
    bound32 = a32.fp32_bound(chunks)[0]
    assert bound32 == (n - 1) * 2.0 ** -24 * exact
    # bf16 accumulation: 2^-9 is a quarter of bf16's ulp at 1.0, every add rounds back to 1.0
    acc = chunks[0]
    for c in chunks[1:]:
        acc, _ = ao.add_bf16(acc, c)
    err16 = abs(float(a32.widen(acc)[0]) - exact)
    assert float(a32.widen(acc)[0]) == 1.0 and err16 == 7 * 2.0 ** -9
    assert err16 > 1e4 * bound32                                  # four orders of magnitude
    assert err16 <= (n - 1) * 2.0 ** -9 * exact                   # its own bound, with 2^-9
    # fp32 accumulation: exact here, within the bound
    got = a32.accumulate_passes(chunks)
    assert got.dtype == np.float32 and abs(float(got[0]) - exact) <= bound32
    assert float(got[0]) == exact
    # one pass: the bf16 bits themselves
    assert a32.accumulate_passes(chunks[:1]).dtype == np.uint16


def test_fp32_bound_holds_on_random_chunks():
    rng = np.random.default_rng(13)
    for n in (2, 3, 4, 8):
        chunks = [so.f32_to_bf16_bits(rng.standard_normal(4096).astype(np.float32)
                                      * np.float32(2.0 ** -(3 * k))) for k in range(n)]
        got = a32.accumulate_passes(chunks).astype(np.float64)
        assert (np.abs(got - a32.exact_sum(chunks)) <= a32.fp32_bound(chunks)).all()
