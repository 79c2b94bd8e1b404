"""bf16 Adam moments on the CPU: the restatement (tests/_bf16_state_oracle.py) through the C oracle
against the same composition over the numpy restatement, bit for bit; the decay table the beta
guard is derived from; the flat state's layout with bf16 moments; the guard itself.

A NaN need only be a NaN (``_adam_space.canon``); no element is left out.
"""
import numpy as np
import pytest
import torch

import _adam_space as sp
import _bf16_state_oracle as bo
from oracle import c_oracle
from oracle import zero_oracle as zo

POINTS = [k for k, v in sp.GRID.items() if not v.get("amsgrad")]
FORMS = ("f32", "bf16", "split", "split_wide")


def _same(name, a, b, nan_of=None):
    ca, cb = sp.canon(a, nan_of), sp.canon(b, nan_of)
    bad = np.flatnonzero(ca != cb)
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:6]}"


def _one_step(point, cls, form, special=False):
    hp = sp.hp_of(point)
    s = sp.planted(cls, seed=2)
    g = sp.special_grads(s) if special else s["g"]
    m0, v0 = bo.narrow(s["m"]), bo.narrow(s["v"])
    p0 = s["p"]
    g_bits = None
    if form in ("bf16", "split"):
        g_bits = zo.f32_to_bf16_bits(g)
        g = zo.bf16_bits_to_f32(g_bits)
    if form in ("split", "split_wide"):
        hi0, lo0 = sp.split_master(p0)
        p0 = sp.join_master(hi0, lo0)
    g = np.ascontiguousarray(g, np.float32)
    wp, wm, wv = bo.numpy_step(p0, g, m0, v0, hp["step"], **sp.update_kwargs(hp))
    chp = c_oracle.hparams(**hp)
    m, v = m0.copy(), v0.copy()
    if form == "f32":
        p = p0.copy()
        bo.adam_f32(p, g, m, v, chp)
        _same("p", p, wp)
    elif form == "bf16":
        p, pb = p0.copy(), np.zeros(p0.size, np.uint16)
        bo.adam_bf16(p, pb, g_bits, m, v, chp)
        _same("p", p, wp)
        _same("p bf16", pb, zo.f32_to_bf16_bits(wp))
    else:
        hi, lo = hi0.copy(), lo0.copy()
        if form == "split":
            bo.adam_bf16_split(hi, lo, g_bits, m, v, chp)
        else:
            bo.adam_f32grad_split(hi, lo, g, m, v, chp)
        whi, wlo = sp.split_master(wp)
        _same("hi", hi, whi)
        _same("lo", lo, wlo, nan_of=whi)
    _same("m", m, wm)
    _same("v", v, wv)


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", POINTS)
def test_c_composition_equals_numpy_composition(point, cls):
    assert "amsgrad" not in point and len(POINTS) == len(sp.GRID) - 3
    for form in FORMS:
        _one_step(point, cls, form)


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("form", FORMS)
def test_special_gradients(form, cls):
    """NaN, +Inf and -Inf gradients: the NaN moment is stored as a NaN, the Inf one as Inf."""
    _one_step("default", cls, form, special=True)
    _one_step("wd", cls, form, special=True)


def test_overflow_rounds_to_inf_and_nan_stays_nan():
    big = np.array([3.4e38, -3.4e38, np.nan, np.inf, 1.0], np.float32)
    bits = bo.narrow(big)
    assert bits[0] == 0x7F80 and bits[1] == 0xFF80 and (bits[2] & 0x7FFF) > 0x7F80
    assert bits[3] == 0x7F80 and bits[4] == 0x3F80


# ---- the guard's derivation ----------------------------------------------------------------------
def _normal_bf16(n=20000, seed=5):
    """n positive normal bf16 values whose next lower binade is normal too (exponent field 2..254)."""
    rng = np.random.default_rng(seed)
    return ((rng.integers(2, 255, n) << 7) | rng.integers(0, 128, n)).astype(np.uint16)


def test_decay_moves_every_value_at_the_bound_and_none_at_torchs_default():
    bits = _normal_bf16()
    assert len(bits) == 20000
    assert bo.MIN_ONE_MINUS_BETA == 2.0 ** -8
    moved = bo.decays(bits, 1.0 - 2.0 ** -8)
    assert moved.all(), f"{(~moved).sum()} values do not decay at 1 - beta = 2^-8"
    moved = bo.decays(bits, 1.0 - 0.001)
    assert not moved.any(), f"{moved.sum()} values decay at 1 - beta = 0.001"
    for omb in (0.0035, 0.002):
        print(f"1 - beta = {omb}: {bo.decays(bits, 1.0 - omb).mean():.3f} of the values decay")


def test_guard():
    from zero_amd._update import (BF16_STATE_MIN_ONE_MINUS_BETA, check_bf16_state_group,
                                  check_state_dtype)

    assert BF16_STATE_MIN_ONE_MINUS_BETA == bo.MIN_ONE_MINUS_BETA
    ok = dict(beta1=0.9, beta2=0.95, amsgrad=False)
    check_bf16_state_group(ok)
    check_bf16_state_group({**ok, "beta2": 0.99})
    check_bf16_state_group({**ok, "beta1": 0.99609375, "beta2": 0.99609375})
    with pytest.raises(ValueError, match=r"beta2.*0\.99609375"):
        check_bf16_state_group({**ok, "beta2": 0.999})
    with pytest.raises(ValueError, match=r"beta1.*0\.99609375"):
        check_bf16_state_group({**ok, "beta1": 0.999})
    with pytest.raises(ValueError, match="amsgrad"):
        check_bf16_state_group({**ok, "amsgrad": True})
    assert check_state_dtype(None) == torch.float32 == check_state_dtype(torch.float32)
    assert check_state_dtype(torch.bfloat16) == torch.bfloat16
    for bad in (torch.float16, torch.float64, "bf16", 2):
        with pytest.raises(ValueError, match="state_dtype"):
            check_state_dtype(bad)


# ---- the flat state's layout -----------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 5, 6, 8, 1001, 4096])
@pytest.mark.parametrize("split,fp32_master", [(True, False), (False, True), (False, False)])
def test_state_layout_bf16(L, split, fp32_master):
    from zero_amd._update import state_layout

    total, lay = state_layout("adam", L, split=split, fp32_master=fp32_master, carry=False,
                              state_dtype=torch.bfloat16)
    half = (L + 1) // 2  # fp32 words of L 16-bit elements
    pad = lambda w: -(-w // 4) * 4  # noqa: E731
    assert lay["m"] == (0, torch.bfloat16) and lay["v"] == (pad(half), torch.bfloat16)
    want = pad(half) + half
    if fp32_master:
        assert lay["master"] == (pad(want), torch.float32)
        want = pad(want) + L
    if split:
        assert lay["lo"] == (pad(want), torch.int16)
        want = pad(want) + half
    assert total == want
    assert set(lay) == {"m", "v"} | ({"master"} if fp32_master else set()) | ({"lo"} if split else set())
    ends = sorted((off, off + (L if dt == torch.float32 else half)) for off, dt in lay.values())
    for (o, e), (o2, _) in zip(ends, ends[1:] + [(total, 0)]):
        assert o % 4 == 0 and e <= o2  # 16-byte aligned starts, no overlap
    # the fp32 layout is what it was
    t32, l32 = state_layout("adam", L, split=split, fp32_master=fp32_master, carry=False)
    assert (t32, l32) == state_layout("adam", L, split=split, fp32_master=fp32_master,
                                      carry=False, state_dtype=torch.float32)
    n32 = 2 + int(fp32_master)
    assert t32 == n32 * L + (half if split else 0)
    assert l32["m"] == (0, torch.float32) and l32["v"] == (L, torch.float32)
    if fp32_master:
        assert l32["master"] == (2 * L, torch.float32)
    if split:
        assert l32["lo"] == (n32 * L, torch.int16)


def test_state_layout_bf16_refusals():
    from zero_amd._update import state_layout

    with pytest.raises(ValueError):
        state_layout("sgd", 8, split=False, fp32_master=False, carry=False,
                     state_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        state_layout("adam", 8, split=False, fp32_master=False, carry=True,
                     state_dtype=torch.bfloat16)
