"""TEST INFRASTRUCTURE — the hyperparameter grid and the planted states shared by
tests/test_sfadam_oracle.py (CPU: the numpy restatement vs zero_amd.optim.ScheduleFreeAdamW itself)
and tests/test_gpu_sfadam_space.py (the HIP kernels vs the restatement).

Every check is ONE step, or one swap, from a planted (y, z, v, carry), as in tests/_adam_space.py,
whose magnitude classes, special gradients, split-master encoding and NaN canonicalisation are used
as they are: y = its p, z = its m, v = its v.  ``small`` (tests/_sgd_space.py's, denormals and
exact zeros) is for the swap alone, which has no gradient and no v.
"""
from __future__ import annotations

import functools

import numpy as np

import _adam_space as asp
import _sgd_space as sgs
from _adam_space import canon, join_master, special_grads, split_master  # noqa: F401  (re-exported)

F32 = np.float32
N = asp.N  # 8192 + 5: torch's vector body and its scalar tail
DEFAULT = dict(lr_t=2.5e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=7, c=0.3)

# name -> what differs from DEFAULT (keywords of _sfadam_oracle.SfHP and
# zero_amd.kernels.sfadam_hparams)
GRID = {
    "default": {},
    "wd": dict(weight_decay=0.1),
    "wd_big": dict(weight_decay=10.0),
    "maximize": dict(maximize=True),
    "all": dict(weight_decay=0.1, maximize=True),
    # lerp: c >= 0.5 takes ATen's high form (0.5 is the boundary itself), 0.49 the low one
    "c_0": dict(c=0.0),
    "c_1": dict(c=1.0),
    "c_0.5": dict(c=0.5),
    "c_0.49": dict(c=0.49),
    "c_below_half": dict(c=0.49999999),  # a double below 0.5 that is 0.5f: the fp32 value decides
    # the betas enter through a = lr_t (beta1 (1 - c) - 1), beta2 also through v and bc2
    "b2_0": dict(beta2=0.0),
    "b2_0.5": dict(beta2=0.5),
    "b1_0.3": dict(beta1=0.3),
    "b1_0.999": dict(beta1=0.999),
    "eps_0": dict(eps=0.0),
    "eps_1": dict(eps=1.0),
    "lr_0": dict(lr_t=0.0),  # a = -0.0 and neg_lr = -0.0
    "lr_1": dict(lr_t=1.0),
    "step_1": dict(step=1),  # bc2 = 1e-3
    "step_3": dict(step=3),
    "step_1000": dict(step=1000),
    "step_1e6": dict(step=10 ** 6),  # bc2 = 1.0f
}
# eval weight 1 - 1/beta1, train weight 1 - beta1: 0.5 is train's boundary (weight 0.5), 2/3
# eval's (weight -0.5); 1e-3 gives an eval weight of -999
SWAP_BETA1 = (0.9, 0.51, 0.5, 2 / 3, 0.3, 1e-3)
CLASSES = ("normal", "wide")
SWAP_CLASSES = CLASSES + ("small",)


def hp_of(point: str) -> dict:
    return {**DEFAULT, **GRID[point]}


def special_params(state: dict, more=()) -> np.ndarray:
    """The y of ``state`` with +Inf, -Inf and NaN planted at elements 5, 66 and 67, and in that
    order again from each index of ``more`` on.  Without weight decay y enters the step through
    the lerp alone: z and v stay finite there, which an unconditional fma(0, y, n) would not
    leave them."""
    y = state["y"].copy()
    for k, val in enumerate((np.inf, -np.inf, np.nan)):
        for at in ((5, 66, 67)[k],) + tuple(a + k for a in more):
            y[at] = val
    return y


@functools.lru_cache(maxsize=None)
def planted(cls: str, n: int = N, seed: int = 0) -> dict:
    """Read-only fp32 arrays g, y, z, v, carry of one magnitude class (cached: shared by the tests).

    normal, wide: g, v and carry of _adam_space.planted, y its p and z its m.
    small (the swap's alone): y the p of _sgd_space.planted("small"), z its buf; g, v and carry
           are there for the arrays' sake only.
    """
    if cls == "small":
        a = sgs.planted("small", n, seed)
        s = {"g": a["g"], "y": a["p"], "z": a["buf"], "v": np.abs(a["carry"]), "carry": a["carry"]}
    else:
        a = asp.planted(cls, n, seed)
        s = {"g": a["g"], "y": a["p"], "z": a["m"], "v": a["v"], "carry": a["carry"]}
    for a in s.values():
        a.setflags(write=False)
    return s
