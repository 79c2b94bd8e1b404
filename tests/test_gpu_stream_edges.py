"""The streaming kernels (segment copy, in-place scale, fp32 <-> bf16 conversion) where the rest of
the suite does not reach: lengths around every chunk boundary, the special values of both formats
under divisors from 2^127 down to 2^-140, and sizes at which every grid-stride loop goes round a
second time at the default grid (128 workgroups per CU).

Every buffer a kernel writes is carved out of a larger allocation with GUARD sentinel elements on
both sides, placed so that the interior keeps its intended alignment, and the whole allocation is
compared, so a store outside [0, n) shows.  Sizes that depend on the device come from its CU
count, and each test asserts the inequality that makes its loop go round.

References are numpy: the source bytes for the copy, fp32 IEEE division for the scale (rounded to
bf16 by oracle.zero_oracle for bf16), oracle.zero_oracle's rounding for the conversion.  The large
cases use the tile scheme of tests/_stream_tiles.py (checked on the CPU by
tests/test_stream_tiles.py).  Outputs are compared bit for bit; the only licence is that where the
reference is a NaN the output need only be a NaN: neither its payload nor its quiet bit is pinned.
"""
import contextlib
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _stream_tiles as stl
from oracle import zero_oracle as zo

pytestmark = pytest.mark.gpu

TESTS = Path(__file__).resolve().parent
GUARD = 4096  # sentinel elements (bytes for the copy) on either side of every written buffer
SENT = {torch.uint8: 0xA5, torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A}
NP = {torch.uint8: np.uint8, torch.int16: np.uint16, torch.int32: np.uint32}
MALL = 256 << 20  # above this many bytes the kernels pick their non-temporal instance by size
# The copy set reads this once per process; the set's unroll cannot be read back through the ABI,
# so the name lives here alone and test_copy_edges_other_unrolls cannot prove which instance ran.
COPY_UNROLL_ENV = "ZERO_AMD_COPY_UNROLL"


def _cap(gpu):
    """grid_cap(): 128 workgroups per CU."""
    return 128 * torch.cuda.get_device_properties(gpu).multi_processor_count


@contextlib.contextmanager
def _tuned(key, value):
    from zero_amd import _lib

    _lib.call("zs_tune", key, int(value), None)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        _lib.call("zs_tune", key, -1, None)


class Guarded:
    """``n`` elements of an integer dtype between two guards of GUARD sentinel elements; ``shift``
    moves the interior that many elements off 16-byte alignment."""

    def __init__(self, gpu, n, dtype, shift=0):
        self.dtype, self.n, self.lo = dtype, n, GUARD + shift
        self.whole = torch.full((2 * GUARD + shift + n,), SENT[dtype], dtype=dtype, device=gpu)
        self.x = self.whole[self.lo:self.lo + n]
        es = self.whole.element_size()
        assert self.whole.data_ptr() % 16 == 0 and GUARD * es % 16 == 0
        assert self.x.data_ptr() % 16 == shift * es % 16
        assert self.lo >= GUARD and self.whole.numel() - (self.lo + n) >= GUARD

    def guards_intact(self):
        s = SENT[self.dtype]
        return bool((self.whole[:self.lo] == s).all()) and bool((self.whole[self.lo + self.n:] == s).all())

    def check_whole(self, interior, nan=None, what=""):
        """The whole allocation against the sentinel with ``interior`` (numpy bits) inside it;
        ``nan``: mask of the interior elements that need only be a NaN."""
        want = np.full(self.whole.numel(), SENT[self.dtype], NP[self.dtype])
        want[self.lo:self.lo + self.n] = interior
        got = self.whole.cpu().numpy().view(NP[self.dtype])
        ok = got == want
        if nan is not None and nan.any():
            at = self.lo + np.flatnonzero(nan)
            vals = got[at].view(np.float32) if got.itemsize == 4 else zo.bf16_bits_to_f32(got[at])
            assert np.isnan(vals).all(), f"{what}: a NaN came back as a number"
            ok[at] = True
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (f"{what}: {bad.size} elements differ, first at {bad[:5] - self.lo} "
                               f"(interior index): got {got[bad[:5]]} want {want[bad[:5]]}")


def _dev_equal(a, b, step=64 << 20):
    """torch.equal in pieces, so the temporaries stay small."""
    assert a.shape == b.shape and a.dtype == b.dtype
    return all(torch.equal(a[i:i + step], b[i:i + step]) for i in range(0, a.numel(), step))


# =================================================================================================
# segment copy
# =================================================================================================
def copy_edge_lengths(K):
    return [K - 17, K - 16, K - 15, K - 1, K, K + 1, K + 15, K + 16, K + 17, 2 * K - 1, 2 * K,
            2 * K + 1, 4 * K + 16 * 255 + 9]


def copy_edges_case(gpu, K, nt, how):
    """Every length around the chunk K, each copied five ways in one table: both sides 16-byte
    aligned, destination off by 3, source off by 5, zero fill aligned and unaligned.  At least 32
    sentinel bytes separate neighbouring destinations.  Also the entry of _copy_unroll_child.py."""
    from zero_amd.kernels import CopySet, copy_direct

    rng = np.random.default_rng(K)
    lens = copy_edge_lengths(K)
    src_h = rng.integers(0, 256, max(lens) + 8192, dtype=np.uint8)
    src = torch.from_numpy(src_h).to(gpu)
    segs, doff = [], GUARD
    for ln in lens:
        for s_shift, d_shift in ((0, 0), (0, 3), (5, 0), (None, 0), (None, 3)):
            so = None if s_shift is None else 16 * int(rng.integers(0, 256)) + s_shift
            doff = (doff + 15) // 16 * 16 + 32 + d_shift
            segs.append((so, doff, ln))
            doff += ln
    total = doff + GUARD
    dst = torch.full((total,), SENT[torch.uint8], dtype=torch.uint8, device=gpu)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    assert all(so is None or so + ln <= src_h.size for so, _, ln in segs)
    assert all(GUARD <= do and do + ln <= total - GUARD for _, do, ln in segs)
    want = np.full(total, SENT[torch.uint8], np.uint8)
    for so, do, ln in segs:
        want[do:do + ln] = 0 if so is None else src_h[so:so + ln]
    s = [0 if so is None else src.data_ptr() + so for so, _, _ in segs]
    d = [dst.data_ptr() + do for _, do, _ in segs]
    n = [ln for _, _, ln in segs]
    with _tuned(b"copy_nt", nt):
        if how == "set":
            CopySet(s, d, n, bounds=([src], [dst])).run(torch.cuda.current_stream())
        else:
            copy_direct(s, d, n, torch.cuda.current_stream(), bounds=([src], [dst]))
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    if bad.size:
        k = max(i for i, (_, do, _) in enumerate(segs) if do <= bad[0] + 64)
        raise AssertionError(f"K={K} copy_nt={nt} {how}: {bad.size} bytes differ, first at {bad[:5]}; "
                             f"near segment {k} (src, dst, n) = {segs[k]}")


@pytest.mark.parametrize("how", ["set", "direct"])
@pytest.mark.parametrize("nt", [-1, 1])
def test_copy_chunk_edges(gpu, how, nt):
    copy_edges_case(gpu, 16384, nt, how)


@pytest.mark.parametrize("how", ["set", "direct"])
@pytest.mark.parametrize("nt", [-1, 0])  # by size, -1 is the non-temporal instance here
def test_copy_strides_past_the_grid(gpu, how, nt):
    """cap + 12 chunks in three segments: workgroups 0..11 take a second chunk, and their forward
    scan crosses an aligned segment with a ragged end, a zero fill on the byte path and a second
    aligned segment."""
    from zero_amd.kernels import CopySet, copy_direct

    K, cap = 16384, _cap(gpu)
    lens = [(cap // 2) * K + 16 * 37 + 5, 3 * K + 1, (cap // 2 + 7) * K]
    chunks = sum(-(-ln // K) for ln in lens)
    assert chunks == cap + 12 and chunks > cap
    assert 2 * sum(lens) > MALL
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    src = torch.randint(0, 256, (max(lens) + (16 << 20),), dtype=torch.uint8, device=gpu)
    soff = [16 * 4099, None, 16 * 7]
    up16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    d0 = GUARD
    e0 = d0 + lens[0]
    d1 = up16(e0 + 64) + 1
    e1 = d1 + lens[1]
    d2 = up16(e1 + 64)
    e2 = d2 + lens[2]
    total = e2 + GUARD
    dst = torch.full((total,), SENT[torch.uint8], dtype=torch.uint8, device=gpu)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    assert all(so is None or so + ln <= src.numel() for so, ln in zip(soff, lens))
    s = [0 if so is None else src.data_ptr() + so for so in soff]
    d = [dst.data_ptr() + do for do in (d0, d1, d2)]
    with _tuned(b"copy_nt", nt):
        if how == "set":
            CopySet(s, d, lens, bounds=([src], [dst])).run(torch.cuda.current_stream())
        else:
            copy_direct(s, d, lens, torch.cuda.current_stream(), bounds=([src], [dst]))
    assert _dev_equal(dst[d0:e0], src[soff[0]:soff[0] + lens[0]]), "first segment"
    assert not bool(dst[d1:e1].any()), "zero fill"
    assert _dev_equal(dst[d2:e2], src[soff[2]:soff[2] + lens[2]]), "last segment"
    for a, b in ((0, d0), (e0, d1), (e1, d2), (e2, total)):
        assert bool((dst[a:b] == SENT[torch.uint8]).all()), f"sentinel bytes [{a}, {b}) were written"
    peak = torch.cuda.max_memory_allocated(gpu) - base
    print(f"{chunks} chunks, {sum(lens)} bytes, peak device memory {peak / 2 ** 20:.0f} MiB")
    assert peak < 1 << 30


@pytest.mark.parametrize("unroll", [2, 8])
def test_copy_edges_other_unrolls(gpu, unroll):
    """The chunk-edge case at the chunk of the other two compiled unrolls, each in a fresh
    interpreter (the library reads the variable once).  Nothing reports which instance ran: a
    library that ignored the variable would pass this test with the default instance."""
    env = dict(os.environ, PYTHONUNBUFFERED="1", **{COPY_UNROLL_ENV: str(unroll)})
    r = subprocess.run([sys.executable, str(TESTS / "_copy_unroll_child.py"), str(4096 * unroll)],
                       cwd=TESTS.parent, capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"copy edges ok K={4096 * unroll}" in r.stdout, r.stdout[-3000:]


# =================================================================================================
# in-place scale
# =================================================================================================
DIVISORS = {"0.5": 0.5, "1": 1.0, "2": 2.0, "3": 3.0, "6": 6.0, "7": 7.0, "8": 8.0,
            "2^127": 2.0 ** 127, "2^-126": 2.0 ** -126, "2^-127": 2.0 ** -127,
            "2^-128": 2.0 ** -128, "2^-140": 2.0 ** -140}


def _scale(gpu, g, div, nt):
    from zero_amd import _lib

    zs = _lib.ZS_F32 if g.dtype == torch.int32 else _lib.ZS_BF16
    with _tuned(b"scale_nt", nt):
        _lib.call("zs_scale", g.x.data_ptr(), g.n, zs, float(div),
                  torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("div", list(DIVISORS))
@pytest.mark.parametrize("nt", [-1, 1])
def test_scale_bf16_every_pattern(gpu, div, nt):
    """All 65,536 bf16 bit patterns (32 wave steps exactly), and the same with a 1,029-element
    tail for block 0."""
    div = DIVISORS[div]
    for n in (65_536, 65_536 + 1_029):
        bits = np.resize(np.arange(65_536, dtype=np.uint32).astype(np.uint16), n)
        want, nan = stl.scale_ref_bf16(bits, div)
        g = Guarded(gpu, n, torch.int16)
        g.x.copy_(stl.as_int_tensor(bits))
        _scale(gpu, g, div, nt)
        g.check_whole(want, nan, f"bf16 n={n} div={div!r}")


def _f32_inputs():
    """(n, bits) of the fp32 value cases: random bit patterns (every exponent, NaNs included) with
    the specials at the head of the vector part and inside the tail; n = 7 is all tail."""
    rng = np.random.default_rng(17)
    sp = stl.SPECIALS.view(np.uint32)
    n = 5 * 1024 + 1000
    x = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    x[:len(sp)] = sp
    x[5 * 1024 + 300:5 * 1024 + 300 + len(sp)] = sp
    return [(n, x), (7, sp[:7].copy()), (7, sp[7:14].copy())]


@pytest.mark.parametrize("div", list(DIVISORS))
@pytest.mark.parametrize("nt", [-1, 1])
def test_scale_f32_special_values(gpu, div, nt):
    div = DIVISORS[div]
    for n, bits in _f32_inputs():
        assert bits.size == n
        q = stl.scale_ref_f32(bits.view(np.float32), div)
        g = Guarded(gpu, n, torch.int32)
        g.x.copy_(stl.as_int_tensor(bits))
        _scale(gpu, g, div, nt)
        g.check_whole(q.view(np.uint32), np.isnan(q), f"fp32 n={n} div={div!r}")


@functools.lru_cache(maxsize=None)
def _scale_tiles(kind):
    """(input tile, tile / 3) as integer tensors on the host."""
    if kind == "f32":
        tile = stl.make_tile_f32(41)
        ref = stl.scale_ref_f32(tile, 3.0)
        assert not np.isnan(ref).any()
    else:
        tile = stl.make_tile_bf16(42)
        ref, nan = stl.scale_ref_bf16(tile, 3.0)
        assert not nan.any()
    return stl.as_int_tensor(tile), stl.as_int_tensor(ref)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("nt", [-1, 0])  # by size, -1 is the non-temporal instance here
def test_scale_strides_past_the_grid(gpu, kind, nt):
    """More wave steps than the capped grid has waves (4 per workgroup): the first 5 waves take a
    second step; 777 elements of tail for block 0."""
    cap = _cap(gpu)
    span, dtype = (1024, torch.int32) if kind == "f32" else (2048, torch.int16)
    n = 4 * cap * span + 5 * span + 777
    assert n // span > 4 * cap
    g = Guarded(gpu, n, dtype)
    assert n * g.whole.element_size() > MALL
    tile, ref = (t.to(gpu) for t in _scale_tiles(kind))
    stl.fill_repeated(g.x, tile)
    _scale(gpu, g, 3.0, nt)
    bad = stl.mismatches_repeated(g.x, ref)
    assert bad == [], f"{kind} n={n}: elements {bad} differ from x / 3"
    assert g.guards_intact()


# =================================================================================================
# fp32 <-> bf16 conversion
# =================================================================================================
F32, BF16 = torch.float32, torch.bfloat16


def _convert(src, dst, to_bf16, nt=-1):
    from zero_amd.kernels import convert

    with _tuned(b"convert_nt", nt):
        if to_bf16:
            convert(src.x.view(F32), dst.x.view(BF16))
        else:
            convert(src.x.view(BF16), dst.x.view(F32))


@functools.lru_cache(maxsize=None)
def _convert_tiles(to_bf16):
    """(source tile, converted tile) as integer tensors on the host."""
    if to_bf16:
        tile = stl.make_tile_f32(43)
        ref = zo.f32_to_bf16_bits(tile)
    else:
        tile = stl.make_tile_bf16(44)
        ref = zo.bf16_bits_to_f32(tile).view(np.uint32)
    return stl.as_int_tensor(tile), stl.as_int_tensor(ref)


def _convert_large(gpu, n, to_bf16, shift, nt=-1):
    s_dt, d_dt = (torch.int32, torch.int16) if to_bf16 else (torch.int16, torch.int32)
    src, dst = Guarded(gpu, n, s_dt, shift), Guarded(gpu, n, d_dt, shift)
    tile, ref = (t.to(gpu) for t in _convert_tiles(to_bf16))
    stl.fill_repeated(src.x, tile)
    _convert(src, dst, to_bf16, nt)
    bad = stl.mismatches_repeated(dst.x, ref)
    assert bad == [], f"n={n}: elements {bad} differ from the reference"
    assert dst.guards_intact()
    assert stl.mismatches_repeated(src.x, tile) == [] and src.guards_intact(), "the source changed"


@pytest.mark.parametrize("to_bf16", [True, False], ids=["to_bf16", "to_f32"])
@pytest.mark.parametrize("nt", [-1, 0])  # by size, -1 is the non-temporal instance here
def test_convert_vector_strides_past_the_grid(gpu, to_bf16, nt):
    """More 1,024-element wave steps than the capped grid has waves; 517 elements of tail."""
    cap = _cap(gpu)
    n = 4 * cap * 1024 + 3 * 1024 + 517
    assert n // 1024 > 4 * cap and 6 * n > MALL
    _convert_large(gpu, n, to_bf16, 0, nt)


@pytest.mark.parametrize("to_bf16", [True, False], ids=["to_bf16", "to_f32"])
def test_convert_scalar_strides_past_the_grid(gpu, to_bf16):
    """Both buffers one element off alignment: the scalar kernel, one element per thread and trip,
    with more elements than the capped grid has threads."""
    cap = _cap(gpu)
    n = 256 * cap + 1000
    assert n > 256 * cap
    _convert_large(gpu, n, to_bf16, 1)


@pytest.mark.parametrize("n", [1, 7, 8, 1000, 1024, 1025, 4099, 3 * 1024 + 517, 1 << 20])
@pytest.mark.parametrize("offset,nt", [(0, -1), (0, 1), (1, -1)])
def test_convert_small_sizes_guarded(gpu, n, offset, nt):
    """The sizes and inputs of test_gpu_kernels.test_convert_fp32_bf16_bit_exact (NaN included)
    with guards around source and destination, both directions."""
    rng = np.random.default_rng(n + offset)
    x = stl.wide_random(rng, n)
    k = min(len(stl.SPECIALS), n)
    x[:k] = stl.SPECIALS[:k]
    nan = np.isnan(x)
    src, dst = Guarded(gpu, n, torch.int32, offset), Guarded(gpu, n, torch.int16, offset)
    src.x.copy_(stl.as_int_tensor(x))
    _convert(src, dst, True, nt)
    dst.check_whole(zo.f32_to_bf16_bits(x), nan, f"fp32 -> bf16 n={n}")
    src.check_whole(x.view(np.uint32), None, "the fp32 source")
    # and back, from what the kernel wrote (bf16 -> fp32 is exact)
    h = dst.x.cpu().numpy().view(np.uint16).copy()
    back = Guarded(gpu, n, torch.int32, offset)
    _convert(dst, back, False, nt)
    back.check_whole(zo.bf16_bits_to_f32(h).view(np.uint32), nan, f"bf16 -> fp32 n={n}")
    dst.check_whole(h, None, "the bf16 source")
