"""Inputs of tests/test_gpu_zero3_clip.py and tests/test_gpu_skip_nonfinite.py (no GPU needed):
exactly known gradients for ZeRO-3 probe models, and what the gradient chunk arena must hold.

A probe module's forward is ``(weight * c).sum()``, so the gradient of ``weight`` is ``c`` bit for
bit.  ``c`` is an integer hash of (step, pass, rank, parameter, element) in [-42, 42] times 2^-8
times the step's scale: x1, x40 and x0.05, so that with ``max_grad_norm`` four times the first
step's norm the clip coefficients are exactly 1, about 0.1 and exactly 1.  x40 and x0.05 are no
powers of two, so a sum over ranks is rounded; the cases run at one or two contributing ranks,
where the sum has two terms at most and one value under any order: fp32(a + b), rounded to bf16
(nearest even) where the exchange is bf16 -- which is what ``reduced`` restates.
"""
import numpy as np

import _accum_oracle as ao
from oracle import zero_oracle as zo

SHAPES = [(66, 128), (7, 24), (16,), (1,)]
SCALES = (1.0, 40.0, 0.05)


def ints(step, pas, rank, mod, shapes=SHAPES):
    n = int(np.prod(shapes[mod]))
    e = np.arange(n, dtype=np.uint64)
    h = (e * np.uint64(2654435761) + np.uint64(40503 * (step + 1) + 9176 * (pas + 1)
                                                 + 65599 * (rank + 1) + 31337 * (mod + 1)))
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(13))) % np.uint64(85)
    return h.astype(np.int64) - 42


def local(step, pas, rank, mod, arena, shapes=SHAPES):
    """One rank's gradient of module ``mod`` (full shape) as fp32 values; ``arena`` "bf16": values
    a bf16 tensor holds exactly."""
    g = (ints(step, pas, rank, mod, shapes) * (2.0 ** -8 * SCALES[step])).astype(np.float32)
    if arena == "bf16":
        g = zo.bf16_bits_to_f32(zo.f32_to_bf16_bits(g))
    return g.reshape(shapes[mod])


def reduced(step, pas, mod, ranks, arena, shapes=SHAPES):
    """What the reduce-scatter delivers for module ``mod`` (full shape, flat): the sum over
    ``ranks`` (one or two) in the arena's representation, float32 or bf16 bits."""
    assert 1 <= len(ranks) <= 2
    s = local(step, pas, ranks[0], mod, arena, shapes).reshape(-1)
    if len(ranks) == 2:
        s = (s + local(step, pas, ranks[1], mod, arena, shapes).reshape(-1)).astype(np.float32)
    return zo.f32_to_bf16_bits(s) if arena == "bf16" else s


def accumulated(step, passes, mod, ranks, arena, widen=False, shapes=SHAPES):
    """The gradient the update reads after ``passes`` backward passes: the arena's running sum,
    rounded to the arena's dtype every pass, or -- ``widen``: accumulation_dtype=float32 over bf16
    chunks, two passes or more -- the fp32 sum of the widened bf16 chunks."""
    g = reduced(step, 0, mod, ranks, arena, shapes)
    for pas in range(1, passes):
        nxt = reduced(step, pas, mod, ranks, arena, shapes)
        if widen:
            g = zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g
            g = (g + zo.bf16_bits_to_f32(nxt)).astype(np.float32)
        else:
            g, nan = ao.accumulate(g, nxt)
            assert not nan.any()
    return g


def values(g):
    """float64 values of a gradient in either representation."""
    return (zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g).astype(np.float64)
