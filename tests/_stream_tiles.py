"""Plain helpers of tests/test_gpu_stream_edges.py (no GPU needed to import or to run them;
tests/test_stream_tiles.py checks them on the CPU).

Large buffers are a host-made *tile* repeated to length n: the reference is computed for one tile
in numpy and compared on the device against every repetition and the remainder.  A tile has
T = 1,000,003 elements, a prime, so a repetition starts at a different phase of every wave step,
chunk and workgroup span.
"""
import numpy as np
import torch

from oracle import zero_oracle as zo

T = 1_000_003

# ±0, ±inf, NaN, 2^-149, the largest denormal, FLT_MIN, FLT_MAX, the bf16 overflow edge
# 3.3895314e38 (bf16's largest finite value), the ties 1 + 2^-8 and 1 + 3 * 2^-8; then the last
# fp32 value that still rounds to the edge and the tie that rounds to infinity
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001,
                     0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F7F0000, 0x3F808000, 0x3F818000,
                     0x7F7F7FFF, 0x7F7F8000], np.uint32).view(np.float32)
assert SPECIALS[9] == np.float32(3.3895314e38) and SPECIALS[10] == np.float32(1.0 + 2.0 ** -8)
SPECIALS_NO_NAN = SPECIALS[~np.isnan(SPECIALS)]
# bf16 patterns the rounding of SPECIALS does not reach: smallest and largest denormal, smallest
# normal, largest finite, both signs of the last
SPECIALS_BF16 = np.array([0x0001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x8001], np.uint16)


def wide_random(rng, n):
    """standard_normal * 10**U(-40, 39) in fp32, as test_gpu_kernels._convert_case: every exponent
    from the denormals to overflow (infinities included), never a NaN."""
    with np.errstate(all="ignore"):
        return (rng.standard_normal(n) * 10.0 ** rng.integers(-40, 39, n)).astype(np.float32)


def make_tile_f32(seed, t=T):
    """fp32 tile: wide random values with the specials (minus NaN) at its head and at its end."""
    x = wide_random(np.random.default_rng(seed), t)
    k = len(SPECIALS_NO_NAN)
    x[:k] = SPECIALS_NO_NAN
    x[t - k:] = SPECIALS_NO_NAN
    assert not np.isnan(x).any()
    return x


def make_tile_bf16(seed, t=T):
    """bf16 tile (uint16 bit patterns): the fp32 tile rounded, plus the bf16-only specials."""
    h = zo.f32_to_bf16_bits(make_tile_f32(seed, t))
    k = len(SPECIALS_NO_NAN)
    h[k:k + len(SPECIALS_BF16)] = SPECIALS_BF16
    h[t - k - len(SPECIALS_BF16):t - k] = SPECIALS_BF16
    assert not np.isnan(zo.bf16_bits_to_f32(h)).any()
    return h


def as_int_tensor(a):
    """A numpy array of 4-, 2- or 1-byte elements as a torch integer tensor of the same bits."""
    a = np.ascontiguousarray(a)
    view = {4: np.int32, 2: np.int16, 1: np.uint8}[a.itemsize]
    return torch.from_numpy(a.view(view).copy())


def fill_repeated(dst, tile):
    """dst[i] = tile[i % len(tile)] for a contiguous 1-d ``dst`` (any device, same dtype)."""
    n, t = dst.numel(), tile.numel()
    reps = n // t
    if reps:
        dst[:reps * t].view(reps, t).copy_(tile.expand(reps, t))
    dst[reps * t:].copy_(tile[:n - reps * t])


def mismatches_repeated(buf, tile, rows=64, limit=8):
    """Flat indices i (``limit`` per block of ``rows`` repetitions at the most) with
    buf[i] != tile[i % len(tile)]: ``torch.equal`` on integer views, block by block so the
    temporaries stay small, every repetition and the remainder; [] when all is equal."""
    assert not buf.dtype.is_floating_point and buf.dtype == tile.dtype
    n, t = buf.numel(), tile.numel()
    reps = n // t
    blocks = [(r0, min(reps, r0 + rows)) for r0 in range(0, reps, rows)]
    pairs = [(r0 * t, buf[r0 * t:r1 * t].view(r1 - r0, t), tile.expand(r1 - r0, t))
             for r0, r1 in blocks]
    pairs.append((reps * t, buf[reps * t:], tile[:n - reps * t]))  # the remainder
    bad = []
    for start, got, want in pairs:
        if not torch.equal(got, want):
            idx = (got != want).flatten().nonzero().flatten()[:limit] + start
            bad += [int(i) for i in idx.tolist()]
    return bad


# ---- numpy references ---------------------------------------------------------------------------
def scale_ref_f32(x, div):
    """x / div in fp32 IEEE division (numpy), overflow and invalid allowed."""
    assert np.float32(2.0 ** -149) / np.float32(2.0 ** -128) == 2.0 ** -21, "numpy flushed a denormal"
    with np.errstate(all="ignore"):
        q = np.asarray(x, np.float32) / np.float32(div)
    assert q.dtype == np.float32
    return q


def scale_ref_bf16(bits, div):
    """(bf16 bits of RNE(widened / div), mask of the elements whose quotient is NaN)."""
    q = scale_ref_f32(zo.bf16_bits_to_f32(bits), div)
    return zo.f32_to_bf16_bits(q), np.isnan(q)
