"""The tile builder and the repetition compare of tests/_stream_tiles.py, on the CPU: what the large
cases of tests/test_gpu_stream_edges.py rest on must itself notice one wrong element."""
import numpy as np
import torch

import _stream_tiles as stl
from oracle import zero_oracle as zo


def test_tile_fill_and_compare_flag_a_planted_element():
    t = stl.T
    n = 2 * t + 12_345  # two repetitions and a remainder
    for tile in (stl.make_tile_f32(3), stl.make_tile_bf16(3)):
        assert tile.size == t
        dev_tile = stl.as_int_tensor(tile)
        buf = torch.zeros(n, dtype=dev_tile.dtype)
        stl.fill_repeated(buf, dev_tile)
        want = np.resize(tile, n)  # numpy's own restatement: tile[i % t]
        assert np.array_equal(buf.numpy().view(tile.dtype), want)
        assert stl.mismatches_repeated(buf, dev_tile) == []
        assert stl.mismatches_repeated(buf, dev_tile, rows=1) == []
        for at in (0, t - 1, t, t + 5, 2 * t - 1, 2 * t, n - 1):  # every repetition, the remainder
            keep = buf[at].item()
            buf[at] ^= 1  # one bit of one element
            assert stl.mismatches_repeated(buf, dev_tile) == [at]
            assert stl.mismatches_repeated(buf, dev_tile, rows=1) == [at]
            buf[at] = keep
        assert stl.mismatches_repeated(buf, dev_tile) == []
        # a buffer one element short of a repetition boundary, and one shorter than a tile
        assert stl.mismatches_repeated(buf[:2 * t - 1], dev_tile) == []
        assert stl.mismatches_repeated(buf[1:t], dev_tile) != []


def test_tiles_hold_the_specials_and_no_nan():
    f = stl.make_tile_f32(1)
    h = stl.make_tile_bf16(1)
    assert not np.isnan(f).any() and not np.isnan(zo.bf16_bits_to_f32(h)).any()
    fb, sb = f.view(np.uint32), stl.SPECIALS_NO_NAN.view(np.uint32)
    assert np.isin(sb, fb[:16]).all() and np.isin(sb, fb[-16:]).all()
    assert np.isin(stl.SPECIALS_BF16, h).all()
    assert np.isin(zo.f32_to_bf16_bits(stl.SPECIALS_NO_NAN), h).all()
    # the random part spans the exponent range: denormals, both infinities' neighbours
    e = (fb >> 23) & 0xFF
    assert (e == 0).sum() > 100 and (e > 0xF0).sum() > 100 and len(np.unique(e)) > 250


def test_scale_reference_keeps_denormals():
    """numpy's fp32 division neither flushes denormal inputs nor denormal results."""
    assert np.float32(2.0 ** -149) / np.float32(2.0 ** -128) == 2.0 ** -21
    q = stl.scale_ref_f32(np.array([2.0 ** -149, 1.0, 2.0 ** -126], np.float32), 2.0 ** -140)
    assert list(q) == [2.0 ** -9, np.inf, 2.0 ** 14]
    q = stl.scale_ref_f32(np.array([1.0, 3.0], np.float32), 2.0 ** 127)
    assert list(q.view(np.uint32)) == [1 << 22, 3 << 22]  # 2^-127 (denormal) and 1.5 * 2^-126
    bits, nan = stl.scale_ref_bf16(np.array([0x7FC0, 0x3F80, 0x0000, 0x7F80], np.uint16), 3)
    assert list(nan) == [True, False, False, False]
    assert bits[1] == 0x3EAB and bits[3] == 0x7F80  # 1/3 = 0x3EAAAAAB rounds up
