"""The SGD oracle (tests/_sgd_oracle.py) itself: its exact fp32 fma against libm's fmaf and its
restated update against torch.optim.SGD on the CPU, both bit for bit (no GPU needed); the latter
again over the hyperparameter and magnitude space of tests/_sgd_space.py, one step from a planted
state, with the library's hyperparameter struct and what the planted inputs reach."""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

import _sgd_oracle as so
import _sgd_space as ss

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


# ---- the hyperparameter and magnitude space of tests/_sgd_space.py ------------------------------
CLIP_COEF = F32(0.3)  # 0x3E99999A: no power of two, so g * coef rounds


def _torch_step(p, g, buf, kw, first, coef=None):
    """One step of live torch.optim.SGD(foreach=False) from the planted state: (p, buffer or None).
    ``first``: the state stays empty, as on torch's own first step."""
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.SGD([tp], foreach=False, **kw)
    tp.grad = torch.from_numpy(g.copy())
    if coef is not None:  # clip_grad_norm_'s g.mul_(clip_coef_clamped), in fp32
        tp.grad.mul_(torch.tensor(coef))
    if not first and kw.get("momentum"):
        opt.state[tp]["momentum_buffer"] = torch.from_numpy(buf.copy())
    opt.step()
    tb = opt.state[tp].get("momentum_buffer")
    return tp.detach().numpy(), None if tb is None else tb.numpy()


def _same(got, want):
    return np.array_equal(ss.canon(np.ascontiguousarray(got, F32)),
                          ss.canon(np.ascontiguousarray(want, F32)))


def _against_torch(point, cls, first, special, coef=None):
    kw = ss.GRID[point]
    s = ss.planted(cls)
    assert s["g"].size == 8192 + 5
    g = ss.special_grads(s) if special else s["g"]
    mom = ss.has_momentum(point)
    p, buf, _ = so.step_f32(s["p"], g, s["buf"] if mom else None, so.SgdHP(first=first, **kw),
                            coef=coef)
    tp, tb = _torch_step(s["p"], g, s["buf"], kw, first, coef)
    assert _same(p, tp)
    if mom:
        assert _same(buf, tb)
    else:
        assert tb is None and buf is None
    return s, g, p, buf


@pytest.mark.parametrize("cls", ss.CLASSES)
@pytest.mark.parametrize("point", list(ss.GRID))
def test_space_matches_torch_sgd_cpu(point, cls):
    """One step from the planted buffer (first=False; on FIRST_POINTS from an empty state too,
    first=True), with and without NaN / +Inf / -Inf gradients: p and the buffer bit for bit, a NaN
    need only be a NaN."""
    for first in (False, True) if point in ss.FIRST_POINTS else (False,):
        for special in (False, True):
            _against_torch(point, cls, first, special)


@pytest.mark.parametrize("cls", ss.CLASSES)
@pytest.mark.parametrize("point", ["mom0.9", "nesterov_wd_max", "all"])
def test_clip_matches_torch_sgd_cpu(point, cls):
    """sgd_elem(coef=c) is torch's step on the gradient multiplied by c in fp32."""
    _against_torch(point, cls, False, True, coef=CLIP_COEF)


@pytest.mark.parametrize("cls", ss.CLASSES)
@pytest.mark.parametrize("point", ["mom0.9", "nesterov_wd_max", "mom0"])
def test_carry_is_the_step_on_the_averaged_gradient(point, cls):
    """No torch counterpart: sgd_elem(carry=...) equals sgd_elem on the gradient of the module
    docstring's formula, computed apart here, and returns that gradient as the new carry; with a
    true division (3, carry_mul 2) and a reciprocal multiply (2, carry_mul 1)."""
    for div, mul in ((3.0, 2.0), (2.0, 1.0)):
        _carry_case(point, div, mul, cls)


def _carry_case(point, div, mul, cls):
    kw = ss.GRID[point]
    s = ss.planted(cls)
    g = ss.special_grads(s)
    buf = s["buf"] if ss.has_momentum(point) else None
    with np.errstate(all="ignore"):
        summed = g + F32(mul) * s["carry"]
        assert summed.dtype == F32
        avg = summed * F32(1.0 / div) if div == 2.0 else summed / F32(div)
        assert avg.dtype == F32
    p, b, c = so.sgd_elem(g, s["p"], buf, so.SgdHP(grad_div=div, carry_mul=mul, **kw),
                          carry=s["carry"])
    pw, bw, cw = so.sgd_elem(avg, s["p"], buf, so.SgdHP(**kw))
    assert cw is None and _same(c, avg) and _same(p, pw)
    assert (b is None and bw is None) if buf is None else _same(b, bw)
    assert (ss.canon(c) != ss.canon(g)).mean() > 0.9  # the carry and the division did something


@pytest.mark.parametrize("point", list(ss.GRID))
def test_hparams_struct_equals_the_oracles(point):
    """zs_sgd_hparams_init (the library loads without a GPU) against SgdHP: every float field bit
    for bit, the three flags, over grad_div 1, 2, 3, 6 and 0.5 and a carry_mul fp32 has to round."""
    from zero_amd.kernels import sgd_hparams

    bits = lambda x: F32(x).view(np.uint32)  # noqa: E731
    kw = ss.GRID[point]
    for div in (1, 2, 3, 6, 0.5):
        for first in (False, True):
            got = sgd_hparams(first=first, grad_div=div, carry_mul=1 / 3, **kw)
            want = so.SgdHP(first=first, grad_div=div, carry_mul=1 / 3, **kw)
            for name, ref in (("neg_lr", want.neg_lr), ("momentum", want.momentum),
                              ("one_minus_dampening", want.omd), ("weight_decay", want.wd),
                              ("grad_div", want.grad_div), ("carry_mul", want.carry_mul)):
                assert bits(getattr(got, name)) == bits(ref), (name, div)
            assert (got.nesterov, got.maximize, got.first) == \
                (int(want.nesterov), int(want.maximize), int(first))
    if point == "lr_0":  # -0.0, not +0.0: p = fma(-0, inf, p) is NaN either way, the bits differ
        assert bits(got.neg_lr) == 0x80000000 == bits(want.neg_lr)
    if point == "damp1.5":
        assert got.one_minus_dampening == -0.5
    if point == "mom_tiny":
        assert got.momentum > 0  # 1e-30 is a normal fp32


# ---- the planted inputs reach what they are meant to reach (the reference alone) ----------------
def _ref(point, cls, special=False):
    s = ss.planted(cls)
    g = ss.special_grads(s) if special else s["g"]
    p, buf, _ = so.step_f32(s["p"], g, s["buf"] if ss.has_momentum(point) else None,
                            so.SgdHP(**ss.GRID[point]))
    return s, g, p, buf


@pytest.mark.parametrize("point,big", [("lr_1e3", 230), ("mom0.9", 1)])
def test_wide_drives_the_parameter_to_inf_nan_and_past_2_64(point, big):
    """With the special gradients p holds +Inf, -Inf and NaN; lr_1e3 overflows on its own as well
    (3e38 * 1e3).  Finite |p| > 2^64: 461 elements (5.6 %) at lr_1e3, 2 at mom0.9 (the planted
    2^65 gradients) measured; the bounds are half of that."""
    _, _, p, _ = _ref(point, "wide", special=True)
    assert (p == np.inf).any() and (p == -np.inf).any() and np.isnan(p).any()
    assert (np.isfinite(p) & (np.abs(p) > 2.0 ** 64)).sum() >= big
    if point == "lr_1e3":
        _, _, p, _ = _ref(point, "wide")
        assert (p == np.inf).any() and (p == -np.inf).any() and not np.isnan(p).any()


def test_small_keeps_the_parameter_among_the_denormals():
    """small, mom0.9.  Measured: 56.8 % of the planted p and 20.9 % of the reference p are non-zero
    denormals (the step adds lr * buf with buf up to 2^-100, which lifts two thirds of them out),
    96.2 % of p changed, 24.7 % of the reference buffer is denormal.  Bounds: half of each."""
    s, _, p, buf = _ref("mom0.9", "small")
    assert ss.is_denormal(s["p"]).mean() > 0.28
    assert ss.is_denormal(p).mean() > 0.10
    assert (p.view(np.uint32) != s["p"].view(np.uint32)).mean() > 0.5
    assert ss.is_denormal(buf).mean() > 0.12
    assert (s["p"] == 0).any() and (s["g"] == 0).any()  # and some exact zeros


def test_mom_tiny_underflows_the_old_buffer():
    """momentum = 1e-30: buf * momentum is an exact zero for 96.1 % of the non-zero planted buffer
    in small and 17.2 % in wide (measured; bounds half of that), while the new buffer, the gradient
    then, is non-zero in 96.5 % / 99.9 %."""
    for cls, share in (("small", 0.48), ("wide", 0.085)):
        s, _, _, buf = _ref("mom_tiny", cls)
        with np.errstate(all="ignore"):
            old = s["buf"] * F32(1e-30)
        assert ((old == 0) & (s["buf"] != 0)).mean() > share
        assert (buf != 0).mean() > 0.48


@pytest.mark.parametrize("cls", ss.CLASSES)
def test_damp1_takes_nothing_of_a_finite_gradient(cls):
    """dampening = 1: buf = fma(0, g, buf * momentum) is buf * momentum wherever g is finite and
    NaN where it is not (0 * inf).  Equal as numbers: where buf * momentum underflows to -0 the
    sum with 0 * g = +0 is +0 (87 elements in small), which the bit comparisons elsewhere hold."""
    s, g, _, buf = _ref("damp1", cls, special=True)
    with np.errstate(all="ignore"):
        old = s["buf"] * F32(0.9)
    fin = np.isfinite(g)
    assert (~fin).sum() == 3 and np.isnan(buf[~fin]).all()
    assert np.array_equal(buf[fin], old[fin])
    flipped = (np.signbit(buf) != np.signbit(old))[fin].sum()
    assert (flipped >= 40) if cls == "small" else True
