"""TEST INFRASTRUCTURE — the hyperparameter grid and the planted states shared by
tests/test_sgd_oracle.py (CPU: the numpy restatement vs live torch) and
tests/test_gpu_sgd_space.py (the HIP kernels vs the restatement).

Every check is ONE step from a planted (p, buf, carry), as in tests/_adam_space.py, whose magnitude
classes, special gradients, split-master encoding and NaN canonicalisation are used as they are.
SGD's parameter takes the gradient's magnitude (p = fma(-lr, g, p)), so a wide gradient drives p
through every exponent, into Inf and NaN, and a small one leaves it among the denormals.
"""
from __future__ import annotations

import functools

import numpy as np

import _adam_space as asp
from _adam_space import canon, join_master, special_grads, split_master  # noqa: F401  (re-exported)

F32 = np.float32
N = asp.N  # 8192 + 5: torch's vector body and its scalar tail

# name -> keywords of _sgd_oracle.SgdHP, zero_amd.kernels.sgd_hparams and torch.optim.SGD
GRID = {
    "mom0": dict(lr=0.1),
    "mom0.9": dict(lr=0.05, momentum=0.9),
    "damp0.1": dict(lr=0.05, momentum=0.9, dampening=0.1),
    "damp1": dict(lr=0.05, momentum=0.9, dampening=1.0),    # 1 - dampening = 0: 0 * g
    "damp1.5": dict(lr=0.05, momentum=0.9, dampening=1.5),  # 1 - dampening < 0
    "mom1": dict(lr=0.05, momentum=1.0),
    "mom_tiny": dict(lr=0.05, momentum=1e-30),              # buf * momentum underflows
    "nesterov": dict(lr=0.02, momentum=0.8, nesterov=True),
    "nesterov_wd_max": dict(lr=0.02, momentum=0.8, nesterov=True, weight_decay=0.1, maximize=True),
    "wd": dict(lr=0.1, momentum=0.9, weight_decay=1e-2),
    "wd_mom0": dict(lr=0.1, weight_decay=1e-2),
    "wd_big": dict(lr=0.1, weight_decay=10.0),
    "maximize": dict(lr=0.05, momentum=0.9, maximize=True),
    "lr_0": dict(lr=0.0, momentum=0.9),                     # neg_lr = -0.0
    "lr_1": dict(lr=1.0, momentum=0.9),
    "lr_1e3": dict(lr=1e3),
    "all": dict(lr=0.02, momentum=0.9, dampening=0.3, weight_decay=1e-3, maximize=True),
}
# these also run with first=True: the planted buffer is then stale and must not be read
FIRST_POINTS = ("mom0.9", "damp1", "nesterov", "nesterov_wd_max", "wd", "all")
CLASSES = ("normal", "wide", "small")


def has_momentum(point: str) -> bool:
    return GRID[point].get("momentum", 0.0) != 0


@functools.lru_cache(maxsize=None)
def planted(cls: str, n: int = N, seed: int = 0) -> dict:
    """Read-only fp32 arrays g, p, buf, carry of one magnitude class (cached: shared by the tests).

    normal, wide: g, p and carry of _adam_space.planted, buf its m.
    small: p exponents in 2^[-152, -110), g, buf and carry in 2^[-152, -100), all signed: below
           2^-126 that leaves denormals, below 2^-150 exact zeros.
    """
    if cls == "small":
        rng = np.random.default_rng([seed, CLASSES.index(cls)])
        s = {"g": asp._pow2(rng, n, -152, -100, True), "buf": asp._pow2(rng, n, -152, -100, True),
             "p": asp._pow2(rng, n, -152, -110, True), "carry": asp._pow2(rng, n, -152, -100, True)}
    else:
        a = asp.planted(cls, n, seed)
        s = {"g": a["g"], "buf": a["m"], "p": a["p"], "carry": a["carry"]}
    for a in s.values():
        a.setflags(write=False)
    return s


def is_denormal(a) -> np.ndarray:
    """Non-zero fp32 values below 2^-126."""
    a = np.abs(np.asarray(a, F32))
    return (a > 0) & (a < np.finfo(F32).tiny)
