"""Pin the Adam oracles to each other and to live torch over the hyperparameter and magnitude space
(tests/_adam_space.py), one step from a planted state each:

(a) the C oracle (oracle/adam_oracle.c, the twin of the HIP kernels' adam_elem) equals the numpy
    restatement (oracle/zero_oracle.py adam_update, exact fp32 fma) bit for bit: parameter, state
    and carry, in the fp32, bf16 and split-master forms;
(b) the numpy restatement and the C oracle equal ``torch.optim.Adam`` / ``AdamW`` (CPU,
    foreach=False) bit for bit on exp_avg, exp_avg_sq and max_exp_avg_sq;
(c) the parameter cannot be pinned to torch bit for bit (torch's vectorized CPU sqrt is not the
    correctly rounded one), so torch's p' and the oracle's p' are both held to
        |p' - ref64| <= 0.5 ulp32(ref64) + 6 * 2^-24 * |u64|
    where u64 = (neg_step * m') / (sqrt(v') / bc2_sqrt + eps) and ref64 = fl32(p * decay) + u64
    are evaluated in float64 from the fp32 m', v' (vmax' under amsgrad) and the fp32 scalars;
    p * decay is the one fp32 multiply (param.mul_) both sides make before the update.  The 6:
    five fp32 roundings in the update (multiply, sqrt, divide, add, divide), each at most 2^-24
    relative, give 5 to first order; one more is margin for second-order terms.  Measured over this grid:
    at most 3.23 for torch and for the oracle (the test prints each figure).  That torch's own p' is held to the same bound shows the bound is no
    looser than the reference needs.

A NaN need only be a NaN.
"""
import functools

import numpy as np
import pytest
import torch

import _adam_space as sp
from oracle import c_oracle
from oracle import zero_oracle as zo

F32, F64 = np.float32, np.float64
# check (a) also runs the ZeRO averaging and the ZeRO-1 carry (the kernels' CARRY instances)
EXTRA = {"div3": dict(grad_div=3.0), "carry": dict(grad_div=3.0, carry_mul=2.0, carry=True),
         "carry_all_adamw": dict(grad_div=3.0, carry_mul=2.0, carry=True, weight_decay=0.1,
                                 amsgrad=True, maximize=True, decoupled=True)}
POINTS_A = list(sp.GRID) + list(EXTRA)


def _hp(point):
    return {**sp.DEFAULT, **EXTRA[point]} if point in EXTRA else sp.hp_of(point)


def _same(a, b, nan_of=None):
    return np.array_equal(sp.canon(a, nan_of), sp.canon(b, nan_of))


def _bad(name, a, b, nan_of=None):
    bad = np.flatnonzero(sp.canon(a, nan_of) != sp.canon(b, nan_of))
    return f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:6]}"


# ------------------------------------------------------------------------------------------------
# (a) C oracle == numpy restatement
# ------------------------------------------------------------------------------------------------
def _c_vs_numpy(point, cls, form):
    hp = _hp(point)
    with_carry = hp.pop("carry", False)
    grad_div, carry_mul = hp.pop("grad_div", 1.0), hp.pop("carry_mul", 0.0)
    s = sp.planted(cls, seed=1)
    ams = hp["amsgrad"]
    g, p0 = s["g"], s["p"]
    if form != "f32":
        g_bits = zo.f32_to_bf16_bits(g)
        g = zo.bf16_bits_to_f32(g_bits)
    if form == "split":
        hi0, lo0 = sp.split_master(p0)
        p0 = sp.join_master(hi0, lo0)
    # numpy
    out = zo.adam_update(p0, g, s["m"], s["v"], hp["step"], vmax=s["vmax"], grad_div=grad_div,
                         carry=s["carry"] if with_carry else None, carry_mul=carry_mul,
                         **sp.update_kwargs(hp))
    want = dict(zip(("p", "m", "v", "vmax", "carry"), out))
    # C
    chp = c_oracle.hparams(grad_div=grad_div, carry_mul=carry_mul, **hp)
    got = {k: s[k].copy() for k in ("m", "v")}
    got["vmax"] = s["vmax"].copy() if ams else None
    got["carry"] = s["carry"].copy() if with_carry else None
    opt = dict(vmax=got["vmax"], carry=got["carry"])
    if form == "f32":
        got["p"] = p0.copy()
        c_oracle.adam_f32(got["p"], np.ascontiguousarray(g), got["m"], got["v"], chp, **opt)
    elif form == "bf16":
        got["p"], got["pb"] = p0.copy(), np.zeros(p0.size, np.uint16)
        c_oracle.adam_bf16(got["p"], got["pb"], g_bits, got["m"], got["v"], chp, **opt)
        want["pb"] = zo.f32_to_bf16_bits(want["p"])
    else:
        got["hi"], got["lo"] = hi0.copy(), lo0.copy()
        c_oracle.adam_bf16_split(got["hi"], got["lo"], g_bits, got["m"], got["v"], chp, **opt)
        want["hi"], want["lo"] = sp.split_master(want.pop("p"))
    for name, a in got.items():
        if a is None:
            continue
        nan_of = want["hi"] if name == "lo" else None
        if name == "lo":
            assert _same(got["hi"], want["hi"]), _bad(f"{form} hi", got["hi"], want["hi"])
        assert _same(a, want[name], nan_of), _bad(f"{form} {name}", a, want[name], nan_of)


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", POINTS_A)
def test_c_oracle_equals_numpy(point, cls):
    """p, m, v, vmax and carry (hi / lo, and the bf16 copy, where the form has them) in the fp32
    form, with bf16 gradients and an fp32 master, and with the split master."""
    for form in ("f32", "bf16", "split"):
        _c_vs_numpy(point, cls, form)


# ------------------------------------------------------------------------------------------------
# live torch, once per (point, class)
# ------------------------------------------------------------------------------------------------
def _torch_step(hp, s, g):
    p = torch.nn.Parameter(torch.from_numpy(s["p"].copy()))
    cls = torch.optim.AdamW if hp["decoupled"] else torch.optim.Adam
    opt = cls([p], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"],
              weight_decay=hp["weight_decay"], amsgrad=hp["amsgrad"], maximize=hp["maximize"],
              foreach=False)
    st = {"step": torch.tensor(float(hp["step"] - 1)),
          "exp_avg": torch.from_numpy(s["m"].copy()), "exp_avg_sq": torch.from_numpy(s["v"].copy())}
    if hp["amsgrad"]:
        st["max_exp_avg_sq"] = torch.from_numpy(s["vmax"].copy())
    opt.state[p] = st
    p.grad = torch.from_numpy(g.copy())
    opt.step()
    assert float(st["step"]) == hp["step"]
    out = {"p": p.detach().numpy(), "m": st["exp_avg"].numpy(), "v": st["exp_avg_sq"].numpy()}
    if hp["amsgrad"]:
        out["vmax"] = st["max_exp_avg_sq"].numpy()
    return out


def _oracles_step(hp, s, g):
    p, m, v, vmax = zo.adam_update(s["p"], g, s["m"], s["v"], hp["step"], vmax=s["vmax"],
                                   **sp.update_kwargs(hp))
    npy = {"p": p, "m": m, "v": v}
    c = {k: s[k].copy() for k in ("p", "m", "v")}
    if hp["amsgrad"]:
        npy["vmax"], c["vmax"] = vmax, s["vmax"].copy()
    c_oracle.adam_f32(c["p"], np.ascontiguousarray(g), c["m"], c["v"], c_oracle.hparams(**hp),
                      vmax=c.get("vmax"))
    return npy, c


@functools.lru_cache(maxsize=None)
def _one_step(point, cls):
    hp = sp.hp_of(point)
    s = sp.planted(cls, seed=2)
    npy, c = _oracles_step(hp, s, s["g"])
    return hp, s, _torch_step(hp, s, s["g"]), npy, c


# ------------------------------------------------------------------------------------------------
# (b) state == torch, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", list(sp.GRID))
def test_state_equals_torch(point, cls):
    hp, _, t, npy, c = _one_step(point, cls)
    for name in ("m", "v") + (("vmax",) if hp["amsgrad"] else ()):
        assert _same(npy[name], t[name]), _bad(f"numpy {name} vs torch", npy[name], t[name])
        assert _same(c[name], t[name]), _bad(f"C {name} vs torch", c[name], t[name])


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", ["amsgrad", "all_adamw"])
def test_state_equals_torch_nan_inf_amsgrad(point, cls):
    """NaN, +Inf and -Inf gradient elements under amsgrad: torch.maximum keeps the NaN of
    exp_avg_sq in max_exp_avg_sq (fmaxf would return the finite operand)."""
    hp = sp.hp_of(point)
    s = sp.planted(cls, seed=3)
    g = sp.special_grads(s, more=(sp.N - 3,))
    t = _torch_step(hp, s, g)
    npy, c = _oracles_step(hp, s, g)
    nan = np.flatnonzero(np.isnan(g))
    assert nan.size and np.isnan(t["vmax"][nan]).all() and np.isnan(c["vmax"][nan]).all()
    for name in ("m", "v", "vmax"):
        assert _same(npy[name], t[name]), _bad(f"numpy {name} vs torch", npy[name], t[name])
        assert _same(c[name], t[name]), _bad(f"C {name} vs torch", c[name], t[name])


# ------------------------------------------------------------------------------------------------
# (c) the parameter within the float64 bound, torch's and the oracle's alike
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point", list(sp.GRID))
def test_parameter_within_bound_of_float64(point):
    hp, s, t, npy, c = _one_step(point, "normal")
    assert _same(npy["p"], c["p"])
    bc1 = 1 - hp["beta1"] ** hp["step"]
    bc2 = 1 - hp["beta2"] ** hp["step"]
    neg_step, bc2_sqrt, eps = F32(-(hp["lr"] / bc1)), F32(bc2 ** 0.5), F32(hp["eps"])
    decay = F32(1 - hp["lr"] * hp["weight_decay"]) if hp["decoupled"] else F32(1)
    m1 = npy["m"].astype(F64)  # equal to torch's by check (b)
    v1 = (npy["vmax"] if hp["amsgrad"] else npy["v"]).astype(F64)
    tiny = 2.0 ** -100
    with np.errstate(all="ignore"):
        u = (F64(neg_step) * m1) / (np.sqrt(v1) / F64(bc2_sqrt) + F64(eps))
        ref = (s["p"] * decay).astype(F32).astype(F64) + u
        # u = 0 exactly (lr = 0, or m' = 0) stays in: the bound is then the half ulp alone
        ok = (np.isfinite(ref) & (np.abs(ref) >= tiny) & np.isfinite(u)
              & ((u == 0) | (np.abs(u) >= tiny)) & np.isfinite(v1) & (v1 >= tiny))
        ulp = np.ldexp(1.0, np.maximum(np.floor(np.log2(np.abs(ref[ok]))), -126).astype(int) - 23)
    assert ok.mean() >= 0.95, ok.mean()
    unit = 2.0 ** -24 * np.abs(u[ok])
    for who, p1 in (("torch", t["p"]), ("oracle", npy["p"])):
        err = np.abs(p1.astype(F64)[ok] - ref[ok])
        over = np.max(np.where(unit > 0, (err - 0.5 * ulp) / np.where(unit > 0, unit, 1), 0))
        print(f"{point}: {who} p' within 0.5 ulp + {max(over, 0):.2f} * 2^-24 |u|; "
              f"{ok.mean():.3f} of the elements checked")
        bad = np.flatnonzero(err > 0.5 * ulp + 6 * unit)
        assert bad.size == 0, (who, bad.size, bad[:6])
    print(f"{point}: torch p' != oracle p' in {np.mean(t['p'] != npy['p']):.3%} of the elements")
