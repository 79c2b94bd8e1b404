"""tests/_ema_oracle.py against torch on the CPU: ``ema_step`` equals ``torch.lerp`` and the
``AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(d))`` recipe bit for bit (a NaN need only
be a NaN), the special decays behave, and the composed Adam + EMA updates leave the Adam arrays the
existing C oracles leave."""
import numpy as np
import pytest
import torch

import _ema_oracle as eo
from _stream_tiles import SPECIALS, wide_random
from oracle import c_oracle
from oracle import zero_oracle as zo

N = 1 << 18


def _wide_pairs():
    rng = np.random.default_rng(41)
    a, b = wide_random(rng, N), wide_random(rng, N)
    k = len(SPECIALS)
    a[:k], b[k:2 * k] = SPECIALS, SPECIALS  # a special against an ordinary value, both ways
    a[2 * k:3 * k], b[2 * k:3 * k] = SPECIALS, SPECIALS[::-1]  # and against another special
    return a, b


def _near_pairs():
    """An EMA next to its master: the difference is a few ulps to a few percent."""
    rng = np.random.default_rng(42)
    a = (rng.standard_normal(N) * 10.0 ** rng.integers(-6, 3, N)).astype(np.float32)
    b = (a * (1 + rng.standard_normal(N) * 10.0 ** rng.integers(-8, -1, N))).astype(np.float32)
    return a, b


PAIRS = {"wide": _wide_pairs(), "near": _near_pairs()}


@pytest.mark.parametrize("data", sorted(PAIRS))
@pytest.mark.parametrize("decay", eo.DECAYS)
def test_ema_step_is_torch_lerp(decay, data):
    ema, master = PAIRS[data]
    want = torch.lerp(torch.from_numpy(ema), torch.from_numpy(master), 1.0 - decay).numpy()
    bad = eo.same_bits(eo.ema_step(ema, master, decay), want)
    assert bad.size == 0, (decay, data, bad.size, bad[:8])
    # the weight the kernel is handed: 1 - decay in double, rounded to fp32 once
    assert eo.weight(decay) == np.float32(1.0 - decay)


@pytest.mark.parametrize("decay", eo.DECAYS)
def test_averaged_model_recipe(decay):
    """update_parameters once before training (it copies) and once after every step."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))
    avg.update_parameters(model)
    ema = [p.detach().numpy().copy() for p in model.parameters()]
    for got, p in zip(avg.module.parameters(), model.parameters()):
        assert torch.equal(got, p)
    for step in range(4):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn_like(p) * 10.0 ** (-step))
        avg.update_parameters(model)
        ema = [eo.ema_step(e, p.detach().numpy(), decay) for e, p in zip(ema, model.parameters())]
        for got, e in zip(avg.module.parameters(), ema):
            bad = eo.same_bits(got.detach().numpy(), e)
            assert bad.size == 0, (decay, step, bad.size)


def test_special_decays():
    ema, master = PAIRS["near"]
    assert eo.same_bits(eo.ema_step(ema, master, 0.0), master).size == 0  # w = 1: the master
    assert eo.same_bits(eo.ema_step(ema, master, 1.0), ema).size == 0  # w = 0: unchanged
    wide_e, wide_m = PAIRS["wide"]
    finite = np.isfinite(wide_e) & np.isfinite(wide_m)
    with np.errstate(all="ignore"):  # (a difference that overflows is not "finite data")
        finite &= np.isfinite(wide_m - wide_e)
    assert finite.sum() > N // 2
    assert eo.same_bits(eo.ema_step(wide_e, wide_m, 0.0)[finite], wide_m[finite]).size == 0
    # w = 0: fma(0, d, ema) = (+-0) + ema, which is ema -- except that (+0) + (-0) is +0 (torch too)
    kept = eo.ema_step(wide_e, wide_m, 1.0)[finite]
    bad = eo.same_bits(kept, wide_e[finite])
    assert (kept[bad] == 0).all() and (wide_e[finite][bad] == 0).all()
    assert bad.size < 16  # the planted zeros only


def test_ema_follows_the_stored_split_master():
    """At an exact tie under an even bf16 parameter the stored master is 1 ulp from the computed
    one (the 0x7FFF residual); the EMA with decay 0 is the stored one."""
    tie = np.array([0x3C808000], np.uint32).view(np.float32)
    hi, lo = c_oracle.split_master(tie)
    assert lo[0] == 0x7FFF
    stored = c_oracle.join_master(hi, lo)
    assert stored.view(np.uint32)[0] == 0x3C807FFF
    hp = c_oracle.hparams(lr=0.0, step=1)  # a step that moves nothing: the tie is stored again
    g = np.zeros(1, np.float32)
    m, v, ema = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
    p = tie.copy()
    c_oracle.adam_f32(p, g, m, v, hp)
    assert p.view(np.uint32)[0] == 0x3C808000
    h, l = c_oracle.split_master(p)
    assert eo.ema_step(ema, c_oracle.join_master(h, l), 0.0).view(np.uint32)[0] == 0x3C807FFF


@pytest.mark.parametrize("cfg", [dict(), dict(weight_decay=1e-2), dict(weight_decay=1e-2, decoupled=True),
                                 dict(maximize=True)], ids=["plain", "wd", "adamw", "maximize"])
def test_composition_leaves_the_adam_arrays_of_the_c_oracles(cfg):
    """The composed updates (fp32 update on the joined master, stored again) against the C oracle's
    own bf16-gradient entry points, 3 steps, bit for bit; the EMA against ema_step of what they
    store."""
    rng = np.random.default_rng(7)
    n = 5000
    master0 = (rng.standard_normal(n) * 0.02).astype(np.float32)
    master0.view(np.uint32)[:4] = [0x3C808000, 0x3C818000, 0xBC808000, 0x00008000]
    grads = [zo.f32_to_bf16_bits((rng.standard_normal(n) * 1e-2).astype(np.float32)) for _ in range(3)]
    decay = 0.999
    # split
    hi, lo = c_oracle.split_master(master0)
    a = dict(hi=hi.copy(), lo=lo.copy(), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    b = dict(hi=hi.copy(), lo=lo.copy(), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    ema = c_oracle.join_master(hi, lo)
    for t, g in enumerate(grads, 1):
        hp = c_oracle.hparams(step=t, **cfg)
        c_oracle.adam_bf16_split(a["hi"], a["lo"], g, a["m"], a["v"], hp)
        before = ema.copy()
        eo.adam_ema_split(b["hi"], b["lo"], eo.prep(g), b["m"], b["v"], ema, hp, decay)
        for k in a:
            assert eo.same_bits(b[k], a[k], floats=k in ("m", "v")).size == 0, (t, k)
        want = eo.ema_step(before, c_oracle.join_master(a["hi"], a["lo"]), decay)
        assert eo.same_bits(ema, want).size == 0
    # fp32 master + bf16 parameter out
    a = dict(p=master0.copy(), pb=np.zeros(n, np.uint16), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    b = dict(p=master0.copy(), pb=np.zeros(n, np.uint16), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    ema = master0.copy()
    for t, g in enumerate(grads, 1):
        hp = c_oracle.hparams(step=t, **cfg)
        c_oracle.adam_bf16(a["p"], a["pb"], g, a["m"], a["v"], hp)
        eo.adam_ema_master(b["p"], b["pb"], eo.prep(g), b["m"], b["v"], ema, hp, decay)
        for k in a:
            assert eo.same_bits(b[k], a[k], floats=k != "pb").size == 0, (t, k)


def test_prep_is_the_oracles_own_averaging():
    """prep(g, div, coef) then a divisor of 1 equals the numpy oracle's grad_div / clip_coef."""
    rng = np.random.default_rng(9)
    n = 4096
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    g[:3] = [np.nan, np.inf, -np.inf]
    z = np.zeros(n, np.float32)
    for div, coef in ((2.0, None), (3.0, None), (3.0, 0.37), (1.0, 0.5)):
        want = zo.adam_update(p, g, z, z, 2, grad_div=div, clip_coef=coef, weight_decay=1e-2)
        got = zo.adam_update(p, eo.prep(g, div, coef), z, z, 2, weight_decay=1e-2)
        for a, b in zip(got[:3], want[:3]):
            assert eo.same_bits(a, b).size == 0, (div, coef)
