"""zs_accumulate_widen bit for bit against tests/_accum32_oracle.py, in both modes (``a`` given:
dst = a + src; ``a`` NULL: dst += src) and both cache policies: lengths around the 256-element
block and the 1,024-element wave step, every bf16 code against the eight sources, the special
values, and a size at which every wave of the default grid takes two or more steps.

``dst``, ``a`` and ``src`` are carved between sentinel guards (tests/test_gpu_stream_edges.py's
``Guarded``) and the whole allocations are compared: the guards are untouched and ``a`` and ``src``
keep their bits.  Where the oracle's sum is a NaN the output need only be a NaN.
"""
import functools

import numpy as np
import pytest
import torch

import _accum32_oracle as a32
import _accum_oracle as ao
import _stream_tiles as stl
from oracle import zero_oracle as zo
from test_gpu_stream_edges import MALL, Guarded, _cap, _tuned

pytestmark = pytest.mark.gpu

SPAN = 1024  # elements per wave step: 4 blocks of 256 (lane l of block u: elements [256u + 4l, +4))
LENGTHS = [0, 1, 3, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 513]


def _launch(dst, a, src, nt):
    from zero_amd.kernels import accumulate_widen

    with _tuned(b"accumulate_nt", nt):
        accumulate_widen(dst.x.view(torch.float32), src.x.view(torch.bfloat16),
                         a=None if a is None else a.x.view(torch.bfloat16))


def _run_case(gpu, first, x_bits, s_bits, nt, what):
    """``x_bits``: bf16 codes of ``a`` (first mode) or fp32 bits of ``dst`` (second mode)."""
    n = s_bits.size
    dst, src = Guarded(gpu, n, torch.int32), Guarded(gpu, n, torch.int16)
    src.x.copy_(stl.as_int_tensor(s_bits))
    if first:
        a = Guarded(gpu, n, torch.int16)
        a.x.copy_(stl.as_int_tensor(x_bits))
        want = a32.widen_first(x_bits, s_bits)
    else:
        a = None
        dst.x.copy_(stl.as_int_tensor(x_bits))
        want = a32.widen_add(x_bits.view(np.float32), s_bits)
    _launch(dst, a, src, nt)
    dst.check_whole(want.view(np.uint32), np.isnan(want), f"{what}: dst")
    src.check_whole(s_bits, None, f"{what}: src")
    if first:
        a.check_whole(x_bits, None, f"{what}: a")


def _random_bf16(rng, n):
    """Wide random values (every exponent, infinities included) with NaNs and specials mixed in."""
    x = stl.wide_random(rng, n)
    k = min(len(stl.SPECIALS), n)
    at = rng.permutation(n)[:k]
    x[at] = stl.SPECIALS[:k]
    return zo.f32_to_bf16_bits(x)


def _random_f32(rng, n):
    x = stl.wide_random(rng, n)
    k = min(len(stl.SPECIALS), n)
    at = rng.permutation(n)[:k]
    x[at] = stl.SPECIALS[:k]
    return x.view(np.uint32).copy()


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_lengths_around_the_block_and_the_wave_step(gpu, first, nt):
    rng = np.random.default_rng(100 + 2 * nt + first)
    for n in LENGTHS:
        x = _random_bf16(rng, n) if first else _random_f32(rng, n)
        _run_case(gpu, first, x, _random_bf16(rng, n), nt, f"first={first} n={n} nt={nt}")


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_every_bf16_code_against_the_eight_sources(gpu, first, nt):
    """8 x 65,536 pairs (512 wave steps) and the same with a 1,029-element tail for block 0.  Second
    mode: the widened codes plus 2^-8, so dst is no longer bf16-representable."""
    a, s = ao.bf16_table()
    for extra in (0, 1029):
        ab, sb = np.resize(a, a.size + extra), np.resize(s, s.size + extra)
        if first:
            _run_case(gpu, True, ab, sb, nt, f"table +{extra}")
        else:
            d = a32.widen_first(ab, np.full(ab.size, 0x3B80, np.uint16))
            _run_case(gpu, False, d.view(np.uint32), sb, nt, f"table +{extra}")


@pytest.mark.parametrize("nt", [0, 1])
def test_specials(gpu, nt):
    """NaN, +-Inf, Inf - Inf, denormals and +-0, as an all-tail call and in the vector part."""
    codes = np.array([0x7FC0, 0xFFC1, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x007F, 0x0080, 0x0000, 0x8000,
                      0x3F80, 0xBF80, 0x7F7F, 0xFF7F], np.uint16)
    a = np.repeat(codes, codes.size)
    s = np.tile(codes, codes.size)
    want = a32.widen_first(a, s)
    inf, ninf, den, mz = 2, 3, 4, 9
    n = codes.size
    assert np.isnan(want[inf * n + ninf]) and np.isnan(want[0]) and np.isnan(want[n + 5])
    assert want.view(np.uint32)[den * n + den] == 0x00020000          # denormals kept
    assert want.view(np.uint32)[mz * n + mz] == 0x80000000             # -0 + -0 = -0
    assert want.view(np.uint32)[mz * n + mz - 1] == 0x00000000         # -0 + +0 = +0
    assert np.isposinf(want[12 * n + 12])                              # overflow
    for rep in (1, 12):  # 196 elements: tail only; 2,352: two wave steps and a tail
        _run_case(gpu, True, np.tile(a, rep), np.tile(s, rep), nt, f"specials x{rep}, first")
    # second mode: the fp32 specials (both columns) against every source, and fp32 denormals
    d = np.repeat(np.concatenate([ao.F32_SPECIALS[:, 0], ao.F32_SPECIALS[:, 1]]), codes.size)
    s2 = np.tile(codes, d.size // codes.size)
    w2 = a32.widen_add(d.view(np.float32), s2)
    assert np.isnan(w2).any() and (w2.view(np.uint32) == 0x00010001).any()  # 2^-149 + 2^-133
    for rep in (1, 6):
        _run_case(gpu, False, np.tile(d, rep), np.tile(s2, rep), nt, f"specials x{rep}, later")


@functools.lru_cache(maxsize=None)
def _tiles(first):
    """(a or dst tile, src tile, their sum) as integer tensors on the host; no NaN among the sums."""
    s = np.roll(stl.make_tile_bf16(54), 7)
    fs = zo.bf16_bits_to_f32(s)
    if first:
        x = stl.make_tile_bf16(53)
        fx = zo.bf16_bits_to_f32(x)
        # inf + -inf would be a NaN, which the tile comparison cannot allow for: keep the signs
        s = np.where(np.isinf(fx) & np.isinf(fs), x, s)
        ref = a32.widen_first(x, s)
    else:
        x = stl.make_tile_f32(51)
        s = np.where(np.isinf(x) & np.isinf(fs), zo.f32_to_bf16_bits(x), s)
        ref = a32.widen_add(x, s)
    assert not np.isnan(ref).any()
    return stl.as_int_tensor(x), stl.as_int_tensor(s), stl.as_int_tensor(ref)


@pytest.mark.parametrize("nt", [-1, 0])  # by size, -1 is the non-temporal instance here
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_strides_past_the_grid(gpu, first, nt):
    """Twice as many wave steps as the capped grid has waves (4 per workgroup), and five more: every
    wave takes two steps, the first five a third; 777 elements of tail for block 0."""
    cap = _cap(gpu)
    n = 2 * 4 * cap * SPAN + 5 * SPAN + 777
    assert n // SPAN >= 2 * 4 * cap and n % SPAN
    dst, src = Guarded(gpu, n, torch.int32), Guarded(gpu, n, torch.int16)
    assert 8 * n > MALL
    x, s, ref = (t.to(gpu) for t in _tiles(first))
    stl.fill_repeated(src.x, s)
    a = None
    if first:
        a = Guarded(gpu, n, torch.int16)
        stl.fill_repeated(a.x, x)
    else:
        stl.fill_repeated(dst.x, x)
    _launch(dst, a, src, nt)
    bad = stl.mismatches_repeated(dst.x, ref)
    assert bad == [], f"first={first} n={n}: elements {bad} differ from the fp32 sum"
    assert dst.guards_intact()
    assert stl.mismatches_repeated(src.x, s) == [] and src.guards_intact(), "the source changed"
    if first:
        assert stl.mismatches_repeated(a.x, x) == [] and a.guards_intact(), "a changed"
