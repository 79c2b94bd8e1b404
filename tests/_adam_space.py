"""TEST INFRASTRUCTURE — the hyperparameter grid and the planted states shared by
tests/test_adam_oracle.py (CPU: C oracle vs numpy restatement vs live torch) and
tests/test_gpu_adam_space.py (the HIP kernels vs the C oracle).

Every check is ONE step from a planted (p, m, v, vmax, carry): a parameter that differs in its
last bit feeds back into exp_avg through weight decay, so longer runs would compare trajectories
that have legitimately parted.
"""
from __future__ import annotations

import numpy as np

from oracle import zero_oracle as zo

F32 = np.float32
N = 8192 + 5
DEFAULT = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=7,
               decoupled=False, amsgrad=False, maximize=False)

# name -> what differs from DEFAULT (keywords of oracle.c_oracle.hparams)
GRID = {
    "default": {},
    "wd": dict(weight_decay=1e-2),
    "adamw": dict(weight_decay=1e-2, decoupled=True),
    "amsgrad": dict(amsgrad=True),
    "maximize": dict(maximize=True),
    "all_adam": dict(weight_decay=0.1, amsgrad=True, maximize=True),
    "all_adamw": dict(weight_decay=0.1, amsgrad=True, maximize=True, decoupled=True),
    # lerp: |1-beta1| >= 0.5 takes ATen's high form (0.5 is the boundary itself), 0.51 the low one
    "b1_0.5": dict(beta1=0.5),
    "b1_0.3": dict(beta1=0.3),
    "b1_0": dict(beta1=0.0),
    "b1_0.51": dict(beta1=0.51),
    "b1_0.999_b2_0.9": dict(beta1=0.999, beta2=0.9),
    "b2_0": dict(beta2=0.0),
    "b2_0.5": dict(beta2=0.5),
    "eps_0": dict(eps=0.0),
    "eps_1": dict(eps=1.0),
    "lr_0": dict(lr=0.0),
    "lr_1": dict(lr=1.0),
    "step_1": dict(step=1),
    "step_3": dict(step=3),
    "step_1000": dict(step=1000),
    "step_1e6": dict(step=10 ** 6),
}
CLASSES = ("normal", "wide")


def hp_of(point: str) -> dict:
    return {**DEFAULT, **GRID[point]}


def update_kwargs(hp: dict) -> dict:
    """The keywords of zero_oracle.adam_update for one grid point (``step`` is positional)."""
    kw = {k: hp[k] for k in ("lr", "eps", "weight_decay", "decoupled", "amsgrad", "maximize")}
    kw["betas"] = (hp["beta1"], hp["beta2"])
    return kw


def _pow2(rng, n, elo, ehi, signed):
    """(1 + 23 random mantissa bits) * 2^e, e uniform in [elo, ehi); rounded into fp32 (below
    2^-126 that leaves denormals, below 2^-150 zeros)."""
    e = rng.integers(elo, ehi, n)
    mant = 1.0 + rng.integers(0, 1 << 23, n) / float(1 << 23)
    x = np.ldexp(mant, e)
    if signed:
        x = x * rng.choice([-1.0, 1.0], n)
    with np.errstate(all="ignore"):
        return x.astype(F32)


def planted(cls: str, n: int = N, seed: int = 0) -> dict:
    """fp32 arrays g, m, v, vmax, p, carry of one magnitude class.

    normal: g, m (and carry) exponents in 2^[-12, 4), v in 2^[-24, 8).
    wide:   g, m (and carry) in 2^[-75, 62), v in 2^[-150, 124) — the squares' range, denormals
            included; a few exact zeros in g, m and v (one element with all three: 0/0 at eps = 0),
            and four gradients of 2^65 and 3e38 whose square overflows.
    Both: vmax >= v (equal in a quarter of the elements), p in 2^[-10, 3).
    """
    rng = np.random.default_rng([seed, CLASSES.index(cls)])
    glo, ghi, vlo, vhi = (-12, 4, -24, 8) if cls == "normal" else (-75, 62, -150, 124)
    s = {"g": _pow2(rng, n, glo, ghi, True), "m": _pow2(rng, n, glo, ghi, True),
         "v": _pow2(rng, n, vlo, vhi, False), "p": _pow2(rng, n, -10, 3, True),
         "carry": _pow2(rng, n, glo, ghi, True)}
    if cls == "wide":
        z = rng.permutation(n)[:40]
        s["g"][z[:10]] = 0
        s["m"][z[5:20]] = 0
        s["v"][z[8:30]] = 0  # z[8:10]: g = m = v = 0
        s["carry"][z[8:12]] = 0
        s["g"][z[30:34]] = np.array([2.0 ** 65, -2.0 ** 65, 3e38, -3e38], F32)
    with np.errstate(all="ignore"):
        grow = _pow2(rng, n, 0, 3, False)
        grow[rng.random(n) < 0.25] = 1
        s["vmax"] = np.minimum(s["v"].astype(np.float64) * grow, np.finfo(F32).max).astype(F32)
    assert (s["vmax"] >= s["v"]).all()
    return s


def special_grads(state: dict, more=()) -> np.ndarray:
    """The gradient of ``state`` with NaN, +Inf and -Inf planted at elements 3, 64 and 65, and in
    that order again from each index of ``more`` on (the NaN / Inf under amsgrad case)."""
    g = state["g"].copy()
    for at in (3,) + tuple(more):
        g[at] = np.nan
    for at in (64,) + tuple(a + 1 for a in more):
        g[at] = np.inf
    for at in (65,) + tuple(a + 2 for a in more):
        g[at] = -np.inf
    return g


# ---- the split master in numpy (include/zero_amd.h ZS_BF16_SPLIT) ----
def split_master(p):
    u = np.asarray(p, F32).view(np.uint32)
    hi = zo.f32_to_bf16_bits(p)
    d = u - (hi.astype(np.uint32) << 16)
    lo = np.where(d == 0x8000, 0x7FFF, d & 0xFFFF).astype(np.uint16)
    return hi, lo


def join_master(hi, lo):
    u = (np.asarray(hi, np.uint16).astype(np.uint32) << 16) + \
        np.asarray(lo, np.uint16).view(np.int16).astype(np.int32).view(np.uint32)
    return u.view(F32)


def canon(a: np.ndarray, nan_of: np.ndarray | None = None) -> np.ndarray:
    """Bit pattern of ``a`` with every NaN as one pattern (a NaN need only be a NaN).  uint16
    arrays are bf16 bits; ``nan_of`` (bf16 bits) marks the elements of a split residual whose
    master is NaN: their residual carries nothing and reads 0."""
    if a.dtype == np.float32:
        u = a.view(np.uint32).copy()
        u[np.isnan(a)] = 0x7FC00000
        return u
    u = a.view(np.uint16).copy()
    if nan_of is not None:
        u[(nan_of.view(np.uint16) & 0x7FFF) > 0x7F80] = 0
    else:
        u[(u & 0x7FFF) > 0x7F80] = 0x7FC0
    return u
