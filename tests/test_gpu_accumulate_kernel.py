"""zs_accumulate (dst += src) bit for bit against tests/_accum_oracle.py: lengths around the wave
step, the special values of both formats, and one size per dtype at which the grid-stride loop
goes round a second time at the default grid.

``dst`` is carved between sentinel guards (tests/test_gpu_stream_edges.py's ``Guarded``) and the
whole allocation is compared; ``src`` is checked to be unchanged.  Where the oracle's sum is a NaN
the output need only be a NaN.
"""
import functools

import numpy as np
import pytest
import torch

import _accum_oracle as ao
import _stream_tiles as stl
from test_gpu_stream_edges import MALL, Guarded, _cap, _tuned

pytestmark = pytest.mark.gpu

# elements per wave step: 64 lanes x 16 bytes x 4 accesses in flight per stream
SPAN = {"f32": 1024, "bf16": 2048}
DT = {"f32": torch.int32, "bf16": torch.int16}


def _accumulate(dst, src, kind, nt):
    from zero_amd.kernels import accumulate

    view = torch.float32 if kind == "f32" else torch.bfloat16
    with _tuned(b"accumulate_nt", nt):
        accumulate(dst.x.view(view), src.x.view(view))


def _run_case(gpu, kind, d_bits, s_bits, nt, what):
    n = d_bits.size
    dst, src = Guarded(gpu, n, DT[kind]), Guarded(gpu, n, DT[kind])
    dst.x.copy_(stl.as_int_tensor(d_bits))
    src.x.copy_(stl.as_int_tensor(s_bits))
    if kind == "f32":
        want, nan = ao.add_f32(d_bits.view(np.float32), s_bits.view(np.float32))
        want = want.view(np.uint32)
    else:
        want, nan = ao.add_bf16(d_bits, s_bits)
    _accumulate(dst, src, kind, nt)
    dst.check_whole(want, nan, f"{what}: dst")
    src.check_whole(s_bits, None, f"{what}: src")


def _random_bits(rng, kind, n):
    """Wide random values (every exponent, infinities included) with NaNs and specials mixed in."""
    x = stl.wide_random(rng, n)
    k = min(len(stl.SPECIALS), n)
    at = rng.permutation(n)[:k]
    x[at] = stl.SPECIALS[:k]
    if kind == "f32":
        return x.view(np.uint32).copy()
    from oracle import zero_oracle as zo

    return zo.f32_to_bf16_bits(x)


def edge_lengths(K):
    return [0, 1, 15, 16, 17, K - 1, K, K + 1, 2 * K - 1, 2 * K + 1, 4 * K + 777]


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_lengths_around_the_wave_step(gpu, kind, nt):
    rng = np.random.default_rng(SPAN[kind] + nt)
    for n in edge_lengths(SPAN[kind]):
        _run_case(gpu, kind, _random_bits(rng, kind, n), _random_bits(rng, kind, n), nt,
                  f"{kind} n={n} nt={nt}")


@pytest.mark.parametrize("nt", [0, 1])
def test_bf16_every_code_against_the_eight_sources(gpu, nt):
    """8 x 65,536 pairs (256 wave steps) and the same with a 1,029-element tail for block 0."""
    d, s = ao.bf16_table()
    for extra in (0, 1029):
        _run_case(gpu, "bf16", np.resize(d, d.size + extra), np.resize(s, s.size + extra), nt,
                  f"bf16 table +{extra}")


@pytest.mark.parametrize("nt", [0, 1])
def test_specials(gpu, nt):
    """The planted bf16 cases and the fp32 specials, in the vector part and as an all-tail call."""
    d = np.array([ao._b(a) for a, _, _ in ao.BF16_PLANTED], np.uint16)
    s = np.array([ao._b(b) for _, b, _ in ao.BF16_PLANTED], np.uint16)
    want, nan = ao.add_bf16(d, s)
    assert [int(w) for w, (_, _, v) in zip(want, ao.BF16_PLANTED) if not np.isnan(v)] == \
        [int(ao._b(v)) for _, _, v in ao.BF16_PLANTED if not np.isnan(v)]
    _run_case(gpu, "bf16", d, s, nt, "bf16 planted, tail")
    _run_case(gpu, "bf16", np.resize(d, 2 * 2048 + 5), np.resize(s, 2 * 2048 + 5), nt,
              "bf16 planted, vector")
    df, sf = ao.F32_SPECIALS[:, 0].copy(), ao.F32_SPECIALS[:, 1].copy()
    _run_case(gpu, "f32", df, sf, nt, "fp32 specials, tail")
    _run_case(gpu, "f32", np.resize(df, 2 * 1024 + 5), np.resize(sf, 2 * 1024 + 5), nt,
              "fp32 specials, vector")


@functools.lru_cache(maxsize=None)
def _tiles(kind):
    """(dst tile, src tile, their sum) as integer tensors on the host; no NaN among the sums."""
    if kind == "f32":
        a, b = stl.make_tile_f32(51), np.roll(stl.make_tile_f32(52), 7)
        # inf + -inf would be a NaN, which the tile comparison cannot allow for: keep the signs
        b = np.where(np.isinf(a) & np.isinf(b), a, b)
        ref, nan = ao.add_f32(a, b)
    else:
        a, b = stl.make_tile_bf16(53), np.roll(stl.make_tile_bf16(54), 7)
        fa, fb = (ao.zo.bf16_bits_to_f32(x) for x in (a, b))
        b = np.where(np.isinf(fa) & np.isinf(fb), a, b)
        ref, nan = ao.add_bf16(a, b)
    assert not nan.any()
    return stl.as_int_tensor(a), stl.as_int_tensor(b), stl.as_int_tensor(ref)


@pytest.mark.parametrize("nt", [-1, 0])  # by size, -1 is the non-temporal instance here
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_strides_past_the_grid(gpu, kind, nt):
    """More wave steps than the capped grid has waves (4 per workgroup): the first 5 waves take a
    second step; 777 elements of tail for block 0."""
    cap = _cap(gpu)
    span = SPAN[kind]
    n = 4 * cap * span + 5 * span + 777
    assert n // span > 4 * cap
    dst, src = Guarded(gpu, n, DT[kind]), Guarded(gpu, n, DT[kind])
    assert 3 * n * dst.whole.element_size() > MALL
    a, b, ref = (t.to(gpu) for t in _tiles(kind))
    stl.fill_repeated(dst.x, a)
    stl.fill_repeated(src.x, b)
    _accumulate(dst, src, kind, nt)
    bad = stl.mismatches_repeated(dst.x, ref)
    assert bad == [], f"{kind} n={n}: elements {bad} differ from dst + src"
    assert dst.guards_intact()
    assert stl.mismatches_repeated(src.x, b) == [] and src.guards_intact(), "the source changed"
