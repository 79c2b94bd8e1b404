"""The Schedule-Free AdamW restatement (tests/_sfadam_oracle.py) against
zero_amd.optim.ScheduleFreeAdamW itself on fp32 CPU tensors (no GPU needed), over the hyperparameter
and magnitude space of tests/_sfadam_space.py: one step from a planted state, the schedule's host
scalars, the eval() / train() swap, and zs_sfadam_hparams_init against the restatement's scalars.

Every comparison is bit for bit over whole arrays; a NaN need only be a NaN; no tolerance and no
element left out.  The class's docstring is the specification: a difference is a finding.
"""
import itertools

import numpy as np
import pytest
import torch

import _sfadam_oracle as so
import _sfadam_space as sp

F32 = np.float32


def _same(got, want):
    got, want = (sp.canon(np.ascontiguousarray(a, F32).reshape(-1)) for a in (got, want))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {want.size} elements differ, first at {bad[:8]}"


def _class(y, beta1=0.9, **kw):
    from zero_amd.optim import ScheduleFreeAdamW

    p = torch.nn.Parameter(torch.from_numpy(np.array(y, F32)))
    return p, ScheduleFreeAdamW([p], betas=(beta1, kw.pop("beta2", 0.999)), **kw)


def planted_weight_sum(c: float) -> float:
    """With ``weight_lr_power=0`` and ``r=0`` every step weighs 1, whatever the learning rate, so a
    planted ``weight_sum`` of S makes the class form c = 1 / (S + 1).  c = 0 beside a non-zero
    learning rate: an S so large that c rounds to 0.0f."""
    return 1e60 if c == 0 else 1.0 / c - 1.0


def class_step(point, s, g):
    """One step of the class from the planted (y, z, v) at the point's (t, lr_t, c): the arrays
    (y, z, exp_avg_sq) and the group afterwards."""
    hp = sp.hp_of(point)
    p, opt = _class(s["y"], hp["beta1"], beta2=hp["beta2"], lr=hp["lr_t"], eps=hp["eps"],
                    weight_decay=hp["weight_decay"], maximize=hp.get("maximize", False),
                    weight_lr_power=0.0, r=0.0)
    group = opt.param_groups[0]
    group.update(k=hp["step"] - 1, weight_sum=planted_weight_sum(hp["c"]), lr_max=hp["lr_t"])
    opt.state[p].update(step=torch.tensor(float(hp["step"] - 1)),
                        z=torch.from_numpy(s["z"].copy()),
                        exp_avg_sq=torch.from_numpy(s["v"].copy()))
    p.grad = torch.from_numpy(g.copy())
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == hp["step"] == group["k"] and group["lr_t"] == hp["lr_t"]
    assert F32(group["c"]) == F32(hp["c"]), (group["c"], hp["c"])
    return (p.detach().numpy(), st["z"].numpy(), st["exp_avg_sq"].numpy()), group


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", list(sp.GRID))
def test_space_matches_the_class_cpu(point, cls):
    """One step from the planted state, with and without NaN / +Inf / -Inf gradients: y, z and
    exp_avg_sq whole.  The oracle takes the class's own c and lr_t, as the wrappers do."""
    s = sp.planted(cls)
    assert s["g"].size == 8192 + 5  # torch's vector body and its scalar tail
    hp = sp.hp_of(point)
    for special in (False, True):
        g = sp.special_grads(s) if special else s["g"]
        want, group = class_step(point, s, g)
        ohp = so.SfHP(**dict(hp, lr_t=group["lr_t"], c=group["c"]))
        got = so.sfadam_elem(g, s["y"], s["z"], s["v"], ohp)
        for name, a, b in zip(("y", "z", "exp_avg_sq"), got, want):
            try:
                _same(a, b)
            except AssertionError as e:
                raise AssertionError(f"{name}, special={special}: {e}") from None


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", ["default", "c_0.5", "c_1", "wd"])
def test_infinite_parameter_matches_the_class_cpu(point, cls):
    """+Inf, -Inf and NaN planted in y.  Without weight decay the class never multiplies y by the
    decay (``n.add_`` is skipped, not run with alpha = 0): z and exp_avg_sq come out as from a
    finite y.  With it, 0.1 * Inf reaches n and z."""
    s = sp.planted(cls)
    at = [5, 66, 67]
    s = dict(s, y=sp.special_params(s))
    assert np.isposinf(s["y"][5]) and np.isneginf(s["y"][66]) and np.isnan(s["y"][67])
    want, group = class_step(point, s, s["g"])
    got = so.sfadam_elem(s["g"], s["y"], s["z"], s["v"],
                         so.SfHP(**dict(sp.hp_of(point), lr_t=group["lr_t"], c=group["c"])))
    for a, b in zip(got, want):
        _same(a, b)
    y, z, _ = got
    if point == "wd":
        assert not np.isfinite(z[at]).any()
    else:
        plain = so.sfadam_elem(sp.planted(cls)["g"], sp.planted(cls)["y"], s["z"], s["v"],
                               so.SfHP(**sp.hp_of(point)))
        _same(z, plain[1])
        assert np.isfinite(z[at]).all()
        # the high form keeps an infinite y (z + (c - 1)(z - y)); c = 1 (0 * Inf) and the low one
        # (Inf - Inf) make it NaN
        assert (np.isinf(y[at[:2]]) if point == "c_0.5" else np.isnan(y[at[:2]])).all()
        assert np.isnan(y[67])


def test_wide_eps_0_reaches_the_planted_zero_over_zero():
    """g = v = 0 at eps = 0 is 0 / 0: exactly the two planted elements are NaN in y, in the
    restatement as in the class (compared above)."""
    s = sp.planted("wide")
    y, _, _ = so.sfadam_elem(s["g"], s["y"], s["z"], s["v"], so.SfHP(**sp.hp_of("eps_0")))
    both = (s["g"] == 0) & (s["v"] == 0)
    assert both.sum() == 2 and np.array_equal(np.isnan(y), both)
    y, _, _ = so.sfadam_elem(s["g"], s["y"], s["z"], s["v"], so.SfHP(**sp.hp_of("default")))
    assert not np.isnan(y).any()


def test_c_below_half_takes_the_high_form():
    """0.49999999 is below 0.5 as a double and 0.5f in fp32: torch's lerp_ decides on the fp32
    weight, and so must the restatement (a decision on the double gives other bits)."""
    c = sp.GRID["c_below_half"]["c"]
    assert c < 0.5 and F32(c) == F32(0.5)
    s = sp.planted("normal")
    y, z = s["y"], s["z"]
    hi = so.fma32(F32(F32(c) - F32(1)), z - y, z)
    low = so.fma32(F32(c), z - y, y)
    assert (sp.canon(hi) != sp.canon(low)).mean() > 0.1
    _same(so.lerp32(y, z, c), hi)
    _same(torch.from_numpy(y.copy()).lerp_(torch.from_numpy(z.copy()), c).numpy(), hi)


SWEEP = list(itertools.product((0, 1, 4), (0.0, 1.0), (2.0, 0.0), (0.0, 2.5e-3)))


@pytest.mark.parametrize("warmup,r,power,lr", SWEEP)
def test_schedule_equals_schedule_free_advance(warmup, r, power, lr):
    """20 steps: (t, lr_t, c) equal as doubles."""
    from zero_amd.optim import schedule_free_advance

    _, opt = _class(np.zeros(4, F32), lr=lr, warmup_steps=warmup, r=r, weight_lr_power=power)
    group = opt.param_groups[0]
    want = [schedule_free_advance(group) for _ in range(20)]
    got = so.schedule(lr, 20, warmup_steps=warmup, r=r, weight_lr_power=power)
    assert got == want
    assert all(type(x) is float for _, lr_t, c in got for x in (lr_t, c))
    assert (group["k"], group["lr_t"], group["c"]) == want[-1]


@pytest.mark.parametrize("cls", sp.SWAP_CLASSES)
@pytest.mark.parametrize("beta1", sp.SWAP_BETA1, ids=lambda b: f"b1_{b:.4g}")
def test_swap_matches_eval_and_train(beta1, cls):
    """``swap`` against the class's eval(), then train() from eval's result."""
    s = sp.planted(cls)
    p, opt = _class(s["y"], beta1)
    opt.state[p].update(step=torch.tensor(1.0), z=torch.from_numpy(s["z"].copy()),
                        exp_avg_sq=torch.zeros(s["y"].size))
    opt.eval()
    x = so.swap(s["y"], s["z"], beta1, True)
    _same(x, p.detach().numpy())
    assert (sp.canon(x) != sp.canon(s["y"])).mean() > 0.5
    opt.train()
    _same(so.swap(x, s["z"], beta1, False), p.detach().numpy())
    _same(opt.state[p]["z"].numpy(), s["z"])


def test_small_keeps_the_swap_among_the_denormals():
    """small: y and z in 2^[-152, -100).  At beta1 = 0.9 more than a tenth of eval's x are non-zero
    denormals and some are exact zeros (the bounds follow from the exponent ranges: y below 2^-126
    in 26 of its 42 exponents, and x = y - 0.111 (z - y) stays there when z is no larger)."""
    s = sp.planted("small")
    x = so.swap(s["y"], s["z"], 0.9, True)
    tiny = np.finfo(F32).tiny
    assert ((np.abs(x) > 0) & (np.abs(x) < tiny)).mean() > 0.1
    assert (s["y"] == 0).any() and (s["z"] == 0).any()


@pytest.mark.parametrize("point", list(sp.GRID))
def test_hparams_struct_equals_the_oracles(point):
    """zs_sfadam_hparams_init (the library loads without a GPU) against SfHP: every float field bit
    for bit and the flag, over grad_div 1, 2, 3 and 0.5 and a carry_mul fp32 has to round."""
    from zero_amd.kernels import sfadam_hparams

    bits = lambda x: F32(x).view(np.uint32)  # noqa: E731
    hp = sp.hp_of(point)
    for div in (1, 2, 3, 0.5):
        got = sfadam_hparams(grad_div=div, carry_mul=1 / 3, **hp)
        want = so.SfHP(grad_div=div, carry_mul=1 / 3, **hp)
        for name, ref in (("beta2", want.beta2), ("one_minus_beta2", want.omb2), ("bc2", want.bc2),
                          ("eps", want.eps), ("weight_decay", want.wd), ("c", want.c),
                          ("a", want.a), ("grad_div", want.grad_div),
                          ("carry_mul", want.carry_mul)):
            assert bits(getattr(got, name)) == bits(ref), (name, div)
        assert bits(-F32(got.lr_t)) == bits(want.neg_lr)  # the run negates lr_t in fp32
        assert got.maximize == int(want.maximize)
    if point == "lr_0":  # a = 0 * (negative) and -lr_t: both -0.0, not +0.0
        assert bits(got.a) == 0x80000000 == bits(want.a) == bits(want.neg_lr)
        assert bits(got.lr_t) == 0
    if point == "step_1":
        assert got.bc2 == F32(1 - 0.999)
    if point == "step_1e6":
        assert got.bc2 == 1.0
    if point in ("c_0.5", "c_below_half"):
        assert bits(got.c) == bits(0.5)
