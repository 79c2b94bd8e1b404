"""The SGD oracle (tests/_sgd_oracle.py) itself: its exact fp32 fma against libm's fmaf and its
restated update against torch.optim.SGD on the CPU, both bit for bit (no GPU needed)."""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

import _sgd_oracle as so

F32 = np.float32


def _libm_fmaf(a, b, c):
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F32)


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def test_fma32_random_and_cancellation():
    rng = np.random.default_rng(0)
    n = 20000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(F32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(F32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(F32)
    assert np.array_equal(_bits(so.fma32(a, b, c)), _bits(_libm_fmaf(a, b, c)))
    # cancellation: c is -a*b rounded to fp32, and that one or two ulps off
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(F32)
    for k in (0, 1, -2):
        ck = (c.view(np.int32) + k).view(F32)
        assert np.array_equal(_bits(so.fma32(a, b, ck)), _bits(_libm_fmaf(a, b, ck)))


def test_fma32_planted_double_rounding():
    """a = b = 1 + 2^-12: a*b = 1 + 2^-11 + 2^-24 is an exact fp32 tie; c = +-2^-60 decides it.  A
    plain float64 evaluation loses c and rounds to even."""
    x = F32(1 + 2.0 ** -12)
    a = np.array([x, x, -x, -x], F32)
    b = np.array([x, x, x, x], F32)
    c = np.array([2.0 ** -60, -(2.0 ** -60), 2.0 ** -60, -(2.0 ** -60)], F32)
    want = _libm_fmaf(a, b, c)
    lo, hi = F32(1 + 2.0 ** -11), np.nextafter(F32(1 + 2.0 ** -11), F32(2))
    assert np.array_equal(want, np.array([hi, lo, -lo, -hi], F32))  # the sign of c decides
    assert np.array_equal(_bits(so.fma32(a, b, c)), _bits(want))
    plain = so.fma32_plain(a, b, c)
    assert (_bits(plain) != _bits(want)).any()
    assert np.array_equal(plain, np.array([lo, lo, -lo, -lo], F32))  # ties to even, c lost


CONFIGS = [
    dict(lr=0.1),
    dict(lr=0.05, momentum=0.9),
    dict(lr=0.05, momentum=0.9, dampening=0.1),
    dict(lr=0.01, momentum=0.8, nesterov=True),
    dict(lr=0.1, momentum=0.9, weight_decay=1e-2),
    dict(lr=0.1, weight_decay=5e-3),
    dict(lr=0.03, momentum=0.7, maximize=True),
    dict(lr=0.02, momentum=0.9, dampening=0.3, weight_decay=1e-3, maximize=True),
]


@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
def test_restatement_matches_torch_sgd_cpu(cfg):
    """6 steps, lengths 4096 and 4099, two param groups (the second with another lr and, where the
    configuration has one, another momentum): parameters and momentum buffers bit for bit."""
    base = CONFIGS[cfg]
    second = dict(base, lr=base["lr"] * 0.37)
    if base.get("momentum"):
        second["momentum"] = base["momentum"] * 0.5
    rng = np.random.default_rng(cfg)
    ps = [(rng.standard_normal(n) * 0.1).astype(F32) for n in (4096, 4099)]
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = torch.optim.SGD([dict(params=[tp[0]], **base), dict(params=[tp[1]], **second)],
                          lr=1.0, foreach=False)
    bufs = [None, None]
    for step in range(6):
        gs = [(rng.standard_normal(p.size) * 0.3).astype(F32) for p in ps]
        for t, g in zip(tp, gs):
            t.grad = torch.from_numpy(g.copy())
        opt.step()
        for i, c in enumerate((base, second)):
            hp = so.SgdHP(first=step == 0, **c)
            ps[i], bufs[i], _ = so.step_f32(ps[i], gs[i], bufs[i], hp)
            assert np.array_equal(_bits(ps[i]), _bits(tp[i].detach().numpy())), (step, i)
            tb = opt.state[tp[i]].get("momentum_buffer")
            if c.get("momentum"):
                assert np.array_equal(_bits(bufs[i]), _bits(tb.numpy())), (step, i)
            else:
                assert tb is None and bufs[i] is None
