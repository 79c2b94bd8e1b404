"""Inputs of tests/test_gpu_zero3_accumulate.py (no GPU needed): exactly known gradients for a
schedule of steps and passes, and the numpy oracle of what the grad chunk arena must hold.

A probe module's forward is ``(weight * c).sum()``, so the gradient of ``weight`` is ``c`` bit for
bit.  ``c`` is an integer hash of (step, pass, rank, parameter, element) in [-42, 42] times a
per-pass power of two: with ws <= 3 every rank sum (|sum| <= 126, 7 bits) is exact in bf16 and
fp32 under any reduction order, while the passes' scales differ so that *accumulating* them is
inexact in the arena's dtype — the roundings the kernel under test must reproduce.
"""
import numpy as np

import _accum_oracle as ao
from oracle import zero_oracle as zo

SHAPES = [(16, 16), (16,), (7, 24), (1,), (33, 8)]
STEPS, PASSES = 3, 3
SCALES = {"bf16": (2.0 ** -6, 2.0 ** -11, 2.0 ** -15), "f32": (1.0, 2.0 ** -20, 2.0 ** -23)}
SKIP_IN_PASS = (1, 1)   # (module, pass): skipped in the second pass of every step
SKIP_IN_STEP = (2, 1)   # (module, step): skipped for the whole of the second step


def active(step, pas, mod):
    return not ((mod, pas) == SKIP_IN_PASS or (mod, step) == SKIP_IN_STEP)


def coeff_ints(step, pas, rank, mod):
    """The integers in [-42, 42] of one gradient (a multiplicative hash of the five indices)."""
    n = int(np.prod(SHAPES[mod]))
    e = np.arange(n, dtype=np.uint64)
    h = (e * np.uint64(2654435761) + np.uint64(40503 * (step + 1) + 9176 * (pas + 1)
                                                 + 65599 * (rank + 1) + 31337 * (mod + 1)))
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(13))) % np.uint64(85)
    return h.astype(np.int64) - 42


def coeff(step, pas, rank, mod, kind):
    """One rank's gradient of module ``mod`` as fp32 values (exactly representable in bf16 too)."""
    return (coeff_ints(step, pas, rank, mod) * SCALES[kind][pas]).astype(np.float32).reshape(SHAPES[mod])


def rank_sum(step, pas, mod, ws, kind):
    """The exact sum over ranks 0..ws-1 (fp32 values; zeros when the module is skipped).  A
    simulated job whose other ranks contribute zeros is ``ws`` = 1 here."""
    if not active(step, pas, mod):
        return np.zeros(SHAPES[mod], np.float32)
    s = sum(coeff_ints(step, pas, r, mod) for r in range(ws))
    assert np.abs(s).max() <= 126
    return (s * SCALES[kind][pas]).astype(np.float32).reshape(SHAPES[mod])


def to_arena(x, arena):
    """fp32 values as the arena's representation: float32, or uint16 bf16 bits (exact here)."""
    if arena == "f32":
        return np.ascontiguousarray(x, np.float32)
    bits = zo.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32))
    assert np.array_equal(zo.bf16_bits_to_f32(bits), x), "a rank sum is not exact in bf16"
    return bits


def accumulated(step, upto_pass, mod, ws, kind, arena):
    """What the arena holds for module ``mod`` after passes 0..upto_pass of ``step`` (full shape;
    float32 or bf16 bits), and whether any of those passes produced a gradient."""
    g = to_arena(rank_sum(step, 0, mod, ws, kind), arena)
    had = active(step, 0, mod)
    for pas in range(1, upto_pass + 1):
        g, nan = ao.accumulate(g, to_arena(rank_sum(step, pas, mod, ws, kind), arena))
        assert not nan.any()
        had = had or active(step, pas, mod)
    return g, had


def addition_stats(ws, kind, arena):
    """(additions, inexact ones, exact ties) over every accumulating addition of the schedule
    whose two operands are both non-zero, in the arena's dtype."""
    total = inexact = ties = 0
    for step in range(STEPS):
        for mod in range(len(SHAPES)):
            for pas in range(1, PASSES):
                d, _ = accumulated(step, pas - 1, mod, ws, kind, arena)
                s = to_arena(rank_sum(step, pas, mod, ws, kind), arena)
                got, _ = ao.accumulate(d, s)
                if arena == "bf16":
                    d, s, got = (zo.bf16_bits_to_f32(x) for x in (d, s, got))
                d64, s64, g64 = (np.asarray(x, np.float64).reshape(-1) for x in (d, s, got))
                exact = d64 + s64  # (exact in float64: the operands span far fewer than 53 bits)
                live = (d64 != 0) & (s64 != 0)
                err = exact - g64
                total += int(live.sum())
                inexact += int((live & (err != 0)).sum())
                if arena == "bf16":
                    low = np.asarray(exact, np.float32).view(np.uint32) & 0xFFFF
                    assert np.array_equal(np.asarray(exact, np.float32).astype(np.float64), exact)
                    ties += int((live & (low == 0x8000)).sum())
                else:
                    g32 = np.asarray(got, np.float32).reshape(-1)
                    other = np.nextafter(g32, np.where(err > 0, np.inf, -np.inf).astype(np.float32))
                    ties += int((live & (err != 0)
                                 & (np.abs(err) == np.abs(other.astype(np.float64) - exact))).sum())
    return total, inexact, ties
