"""The Lion restatement (tests/_lion_oracle.py) against zero_amd.optim.Lion on fp32 CPU tensors,
bit for bit (no GPU needed): 3 steps, two beta pairs, weight decay on and off, maximize, planted
gradients that make the interpolation c exactly +0 / -0, and NaN / +Inf / -Inf gradients; the
bf16-momentum narrowing; zs_lion_hparams_init against the restatement's scalars; the optimizer's own
argument checks and state_dict round trip."""
import copy

import numpy as np
import pytest
import torch

import _lion_oracle as lo

F32 = np.float32
STEPS = 3


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


CONFIGS = [
    dict(lr=1e-4),
    dict(lr=3e-3, betas=(0.95, 0.98)),
    dict(lr=1e-3, weight_decay=0.1),
    dict(lr=3e-3, betas=(0.95, 0.98), weight_decay=1e-2),
    dict(lr=1e-3, maximize=True),
    dict(lr=2e-3, betas=(0.95, 0.98), weight_decay=0.05, maximize=True),
]


def _hp(cfg, **kw):
    b1, b2 = cfg.get("betas", (0.9, 0.99))
    return lo.LionHP(cfg["lr"], b1, b2, cfg.get("weight_decay", 0.0),
                     maximize=cfg.get("maximize", False), **kw)


def _plant(g, m, hp, step):
    """Gradients that make c = fma(1-b1, g, m*b1) exactly zero, and the non-finite ones.  Where m
    is 0 (every element at step 1, and elements whose momentum was held at 0), g = +-0 gives
    c = +-0: the sign is +0 for both, and p must not move."""
    g[0], g[1] = F32(0.0), F32(-0.0)
    if step > 1:  # g = -m*b1 / (1-b1) in double, rounded: c is zero or a tiny residual of either sign
        with np.errstate(all="ignore"):
            g[2:34] = (-(m[2:34].astype(np.float64) * float(hp.beta1)) / float(hp.omb1)).astype(F32)
    g[40], g[41], g[42] = F32(np.nan), F32(np.inf), F32(-np.inf)
    return g


@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
def test_restatement_matches_lion_cpu(cfg):
    """Lengths 4096 and 4099, two param groups (the second with another lr): parameters and exp_avg
    bit for bit over 3 steps."""
    from zero_amd.optim import Lion

    base = CONFIGS[cfg]
    second = dict(base, lr=base["lr"] * 0.37)
    rng = np.random.default_rng(cfg)
    ps = [(rng.standard_normal(n) * 0.1).astype(F32) for n in (4096, 4099)]
    ps[0][:2] = [0.0, -0.0]
    ms = [np.zeros(p.size, F32) for p in ps]
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = Lion([dict(params=[tp[0]], **base), dict(params=[tp[1]], **second)])
    zero_c = 0
    for step in range(1, STEPS + 1):
        gs = []
        for i, c in enumerate((base, second)):
            g = (rng.standard_normal(ps[i].size) * 0.3).astype(F32)
            gs.append(_plant(g, ms[i], _hp(c), step))
        for t, g in zip(tp, gs):
            t.grad = torch.from_numpy(g.copy())
        opt.step()
        for i, c in enumerate((base, second)):
            hp = _hp(c)
            gg = -gs[i] if hp.maximize else gs[i]
            with np.errstate(all="ignore"):
                cc = lo.fma32(hp.omb1, gg, (ms[i] * hp.beta1).astype(F32))
            zero_c += int((cc == 0).sum())
            ps[i], ms[i], _ = lo.step_f32(ps[i], gs[i], ms[i], hp)
            assert np.array_equal(_bits(ps[i]), _bits(tp[i].detach().numpy())), (step, i)
            st = opt.state[tp[i]]
            assert np.array_equal(_bits(ms[i]), _bits(st["exp_avg"].numpy())), (step, i)
            assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu"
            assert float(st["step"]) == step
    assert zero_c >= 2 * 2 * STEPS  # the planted +-0 gradients over zero momentum, at least
    # the non-finite gradients reached the momentum; the parameter only ever moves by lr
    assert all(np.isfinite(p[40:43]).all() for p in ps)
    assert all(np.isnan(m[40]) and np.isinf(m[41]) and np.isinf(m[42]) for m in ms)


def test_sign_of_zero_and_nan_is_plus_zero():
    c = np.array([0.0, -0.0, np.nan, 1e-45, -1e-45, np.inf, -np.inf], F32)
    want = torch.sign(torch.from_numpy(c)).numpy()
    assert np.array_equal(_bits(lo.sign32(c)), _bits(want))
    assert np.array_equal(_bits(want), _bits(np.array([0, 0, 0, 1, -1, 1, -1], F32)))
    # and p does not move there: fma(-lr, +0, p) == p for every p but the sign of -0 + -0
    hp = lo.LionHP(1e-3)
    p = np.array([1.5, -2.0, 0.0, -0.0], F32)
    got, m, _ = lo.step_f32(p, np.zeros(4, F32), np.zeros(4, F32), hp)
    assert np.array_equal(_bits(got), _bits(p)) and not m.any()


def test_bf16_momentum_narrowing():
    """bf16 momentum: the rule sees the widened code, the parameter comes from the unrounded
    interpolation, and the store rounds to nearest even or with the low half of the element's
    draw."""
    import _bf16_state_sr_oracle as sro

    rng = np.random.default_rng(7)
    n = 1000
    hp = lo.LionHP(1e-3, 0.9, 0.99, 0.01)
    p = (rng.standard_normal(n) * 0.1).astype(F32)
    g = (rng.standard_normal(n) * 0.3).astype(F32)
    m_bits = lo.f32_to_bf16_bits((rng.standard_normal(n) * 0.1).astype(F32))
    m_wide = lo.bf16_bits_to_f32(m_bits)
    p32, m32, _ = lo.step_f32(p, g, m_wide, hp)
    pn, mn, _ = lo.step_f32(p, g, m_bits, hp)
    assert mn.dtype == np.uint16 and np.array_equal(_bits(pn), _bits(p32))
    assert np.array_equal(mn, lo.f32_to_bf16_bits(m32))
    e = np.arange(5, 5 + n, dtype=np.uint64)
    keys = lo.keys_of(1234, 3)
    ps, msr, _ = lo.step_f32(p, g, m_bits, hp, sr=(e, keys))
    assert np.array_equal(_bits(ps), _bits(p32))
    r16 = sro.bits(e, *keys) & np.uint32(0xFFFF)
    assert np.array_equal(msr, ((m32.view(np.uint32).astype(np.uint64) + r16) >> 16).astype(np.uint16))
    down = lo.bf16_bits_to_f32((m32.view(np.uint32) >> 16).astype(np.uint16))
    up = lo.bf16_bits_to_f32(((m32.view(np.uint32) >> 16) + 1).astype(np.uint16))
    got = lo.bf16_bits_to_f32(msr)
    assert ((got == down) | (got == up)).all() and (got == down).any() and (got == up).any()


def test_hparams_struct_equals_the_oracles():
    """zs_lion_hparams_init (the library loads without a GPU) against LionHP: every float field
    bit for bit."""
    from zero_amd.kernels import lion_hparams

    bits = lambda x: F32(x).view(np.uint32)  # noqa: E731
    for cfg in CONFIGS + [dict(lr=0.0), dict(lr=1e-4, betas=(0.0, 0.0))]:
        b1, b2 = cfg.get("betas", (0.9, 0.99))
        for div in (1, 2, 3, 6, 0.5):
            got = lion_hparams(cfg["lr"], b1, b2, cfg.get("weight_decay", 0.0),
                               maximize=cfg.get("maximize", False), grad_div=div, carry_mul=1 / 3)
            want = _hp(cfg, grad_div=div, carry_mul=1 / 3)
            for name, ref in (("neg_lr", want.neg_lr), ("beta1", want.beta1),
                              ("one_minus_beta1", want.omb1), ("beta2", want.beta2),
                              ("one_minus_beta2", want.omb2), ("decay_mul", want.decay_mul),
                              ("grad_div", want.grad_div), ("carry_mul", want.carry_mul)):
                assert bits(getattr(got, name)) == bits(ref), (name, cfg, div)
            assert got.maximize == int(want.maximize)
    assert bits(lion_hparams(0.0).neg_lr) == 0x80000000  # -0.0
    assert lion_hparams(1e-3, weight_decay=0.0).decay_mul == 1.0


def test_lion_refuses_bad_arguments():
    from zero_amd.optim import Lion

    mk = lambda: [torch.nn.Parameter(torch.zeros(3))]  # noqa: E731
    for kw in (dict(lr=-1e-4), dict(betas=(1.0, 0.99)), dict(betas=(-0.1, 0.99)),
               dict(betas=(0.9, 1.0)), dict(betas=(0.9, -0.5)), dict(weight_decay=-1e-2)):
        with pytest.raises(ValueError):
            Lion(mk(), **kw)
    opt = Lion(mk())
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["weight_decay"], g["maximize"]) == (1e-4, (0.9, 0.99), 0.0, False)


def test_lion_closure_and_state_dict_round_trip():
    from zero_amd.optim import Lion

    gen = torch.Generator().manual_seed(3)
    mk = lambda: [torch.nn.Parameter(torch.randn(7, 5, generator=torch.Generator().manual_seed(1))),  # noqa: E731
                  torch.nn.Parameter(torch.randn(11, generator=torch.Generator().manual_seed(2)))]
    a, b = mk(), mk()
    oa = Lion(a, lr=1e-2, weight_decay=0.1)
    grads = [[torch.randn(p.shape, generator=gen) for p in a] for _ in range(4)]

    def run(opt, params, gs):
        for p, g in zip(params, gs):
            p.grad = g.clone()
        return opt.step(lambda: torch.tensor(2.5))

    assert float(run(oa, a, grads[0])) == 2.5
    run(oa, a, grads[1])
    sd = copy.deepcopy(oa.state_dict())  # (as saved: torch's loader keeps the tensors it is given)
    assert set(sd["state"][0]) == {"step", "exp_avg"} and float(sd["state"][0]["step"]) == 2
    ob = Lion(b, lr=1.0)  # other hyper-parameters: the loaded groups replace them
    with torch.no_grad():
        for pb, pa in zip(b, a):
            pb.copy_(pa)
    ob.load_state_dict(sd)
    assert ob.param_groups[0]["lr"] == 1e-2 and ob.param_groups[0]["weight_decay"] == 0.1
    for k in (2, 3):
        run(oa, a, grads[k])
        run(ob, b, grads[k])
    for pa, pb in zip(a, b):
        assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
        assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"])
        assert float(ob.state[pb]["step"]) == 4
