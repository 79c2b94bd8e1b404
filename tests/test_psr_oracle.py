"""Master-free bf16 parameters (``master="none"``, p_dtype ZS_BF16_SR), on the CPU: the keys of the
parameter's draw against the library's host function (zs_sr_pkeys through ctypes), the independence
of the three draws of one element, the unbiasedness that is the reason for the feature, the edge
values of the parameter's store, and what can be refused without a GPU.
"""
import ctypes

import numpy as np
import pytest

import _bf16_state_sr_oracle as so
import _psr_oracle as po
from oracle import c_oracle
from oracle import zero_oracle as zo

U32 = np.uint32
N = 1 << 16
E = np.arange(N, dtype=np.uint64)


def test_host_pkeys_equal_numpy():
    """zs_sr_pkeys against the numpy ``pkeys`` on 4096 key pairs: the edges, keys of real launches
    and random words."""
    from zero_amd import _lib

    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    P32 = ctypes.POINTER(ctypes.c_uint32)
    raw.zs_sr_pkeys.argtypes = [ctypes.c_uint32, ctypes.c_uint32, P32, P32]
    rng = np.random.default_rng(5)
    pairs = [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0x85EBCA6B, 0x3D4D51CB), (1, 0xFFFFFFFF)]
    pairs += [so.keys_of(seed, t) for seed in (0, 1, 0xDEADBEEFCAFEF00D) for t in (1, 2, 1 << 33)]
    pairs += [tuple(int(x) for x in rng.integers(0, 1 << 32, 2)) for _ in range(4096 - len(pairs))]
    assert len(pairs) == 4096
    for k0, k1 in pairs:
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        assert raw.zs_sr_pkeys(k0, k1, ctypes.byref(a), ctypes.byref(b)) == _lib.ZS_OK
        assert (a.value, b.value) == po.pkeys(k0, k1), (k0, k1)
    assert raw.zs_sr_pkeys(0, 0, None, None) == _lib.ZS_ERR_INVALID


def test_wrapper_equals_numpy():
    from zero_amd.kernels import sr_bits, sr_keys, sr_pkeys

    keys = sr_keys(0xDEADBEEFCAFEF00D, 7)
    assert sr_pkeys(keys) == po.pkeys(*keys)
    e = (1 << 32) + 5
    assert sr_bits(e, sr_pkeys(keys)) & 0xFFFF == int(po.r16p(np.array([e], np.uint64), keys)[0])


@pytest.mark.parametrize("seed", [0, 1])
def test_the_three_draws_of_an_element_are_uncorrelated(seed):
    """Elements 0 .. 2^16 - 1 at step 1: the parameter's 16 bits and the m and v halves of the
    same element agree in their top bit in N/2 cases, each pair within 5 sigma (sigma = sqrt(N)/2
    = 128)."""
    keys = so.keys_of(seed, 1)
    r = so.bits(E, *keys)
    top = {"p": po.r16p(E, keys) >> U32(15), "m": (r >> U32(15)) & U32(1), "v": r >> U32(31)}
    for a, b in (("p", "m"), ("p", "v"), ("m", "v")):
        equal = int((top[a] == top[b]).sum())
        print(f"seed {seed}: top bits of {a} and {b} equal in {equal} of {N}")
        assert abs(equal - N // 2) <= 5 * 128, (a, b, equal)
    for name, t in top.items():  # and each is a fair bit
        assert abs(int(t.sum()) - N // 2) <= 5 * 128, name


def test_an_update_of_an_eighth_of_an_ulp_moves_an_eighth_of_the_elements():
    """p = 1.0, g = 1, step 1, beta1 = 0.5, beta2 = 0.75, eps = 0, lr = 2^-11: m' = 0.5,
    sqrt(v') / sqrt(bc2) = 1 and the fp32 result is 1 - 2^-11 exactly, an eighth of the bf16 ulp
    below 1.  Rounded to nearest no parameter ever moves; under the oracle N/8 of them do, within
    5 sigma, sigma = sqrt(N * 1/8 * 7/8) = 84.7."""
    hp = c_oracle.hparams(lr=2.0 ** -11, beta1=0.5, beta2=0.75, eps=0.0, step=1)
    p = np.ones(N, np.float32)
    m, v = np.zeros(N, np.float32), np.zeros(N, np.float32)
    c_oracle.adam_f32(p, np.ones(N, np.float32), m, v, hp)
    assert (p.view(U32) == 0x3F7FE000).all() and p[0] == 1.0 - 2.0 ** -11
    assert (zo.f32_to_bf16_bits(p) == 0x3F80).all()  # to nearest: lost
    for state in po.STATES:
        p_bits = np.full(N, 0x3F80, np.uint16)
        g_bits = np.full(N, 0x3F80, np.uint16)
        z = np.float32 if state == "f32" else np.uint16
        po.step(p_bits, g_bits, np.zeros(N, z), np.zeros(N, z), hp, E, so.keys_of(0, 1), state)
        assert np.isin(p_bits, (0x3F80, 0x3F7F)).all()
        moved = int((p_bits == 0x3F7F).sum())
        print(f"{state}: {moved} of {N} parameters moved (N/8 = {N // 8})")
        assert abs(moved - N // 8) <= 5 * np.sqrt(N * (1 / 8) * (7 / 8)), moved
    mean = po.widen(p_bits).astype(np.float64).mean()
    assert abs(mean - (1.0 - 2.0 ** -11)) < 5 * 84.7 / N * 2.0 ** -8  # the mean is the fp32 result


def test_edge_values_of_the_parameter_store():
    keys = so.keys_of(3, 9)
    r = po.r16p(E, keys)
    # a NaN keeps the nearest conversion's code, whatever its draw; +-Inf stays
    x = np.array([0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0xFFC12345, 0x7F800000, 0xFF800000],
                 U32).view(np.float32)
    for at in (0, 17, 4099):
        e = E[at:at + x.size]
        assert np.array_equal(po.narrow_param(x, e, keys), zo.f32_to_bf16_bits(x))
    # the largest finite bf16 with a low half: Inf when the draw carries, the edge otherwise
    big = np.full(N, 0x7F7F8000, U32).view(np.float32)
    got = po.narrow_param(big, E, keys)
    carry = r >= U32(0x8000)
    assert carry.any() and (~carry).any()
    assert (got[carry] == 0x7F80).all() and (got[~carry] == 0x7F7F).all()
    assert (po.narrow_param(-big, E, keys)[carry] == 0xFF80).all()
    # a low half of 0 is exact under every draw: every bf16 value, denormals and zeros included
    codes = np.arange(N, dtype=np.uint16)
    finite = (codes & 0x7FFF) <= 0x7F80
    assert np.array_equal(po.narrow_param(po.widen(codes), E, keys)[finite], codes[finite])


def test_lr_0_leaves_every_parameter_as_it_is():
    """The rule at lr = 0 returns the widened parameter, whose low half is 0: no draw moves it."""
    hp = c_oracle.hparams(lr=0.0, step=3)
    rng = np.random.default_rng(1)
    p_bits = rng.integers(0, 1 << 16, N).astype(np.uint16)
    p_bits[(p_bits & 0x7FFF) > 0x7F80] = 0x7FC0  # (a signalling NaN is quieted by the arithmetic)
    p_bits[p_bits == 0x8000] = 0  # (-0 + +0 = +0: the rule's own sum)
    before = p_bits.copy()
    g = zo.f32_to_bf16_bits(rng.standard_normal(N).astype(np.float32))
    po.step(p_bits, g, np.zeros(N, np.uint16), np.zeros(N, np.uint16), hp, E, so.keys_of(0, 3),
            "bf16_sr")
    assert np.array_equal(p_bits, before)


# ---- what the host refuses without a GPU ----------------------------------------------------
def test_state_layout_without_a_master():
    import torch

    from zero_amd._update import state_layout

    for sd, words in ((None, 2 * 1001), (torch.bfloat16, 504 + 501)):
        total, lay = state_layout("adam", 1001, master="none", state_dtype=sd)
        assert sorted(lay) == ["m", "v"] and total == words
    assert "lo" in state_layout("adam", 8, split=True, fp32_master=False, carry=False)[1]
    for kw in (dict(kind="sgd"), dict(carry=True), dict(split=True), dict(fp32_master=True)):
        with pytest.raises(ValueError):
            state_layout(kw.pop("kind", "adam"), 8, master="none", **kw)
    with pytest.raises(ValueError):
        state_layout("adam", 8, master="half")


def test_checks_without_a_gpu():
    import torch

    from zero_amd import checkpoint as ckpt
    from zero_amd._update import check_master_free, check_master_free_group

    check_master_free("adam", False, True)
    for args, word in ((("sgd", False, True), "SGD"), (("adam", True, True), "carry"),
                       (("adam", False, False), "bf16 parameters")):
        with pytest.raises(ValueError, match=word):
            check_master_free(*args)
    check_master_free_group({"amsgrad": False})
    with pytest.raises(ValueError, match="amsgrad"):
        check_master_free_group({"amsgrad": True})
    # the header records the master and the seed; neither is compared
    h = ckpt.header(2, 1, 0, [0], state_seed=5, master="none")
    assert h["master"] == "none" and h["state_seed"] == 5
    assert "master" not in ckpt.header(2, 1, 0, [0])
    ckpt.check_header({"zero_amd": h}, ckpt.header(2, 1, 0, [0], master="split"))
    # an entry with a master cannot be loaded into an optimizer that keeps none
    z = torch.zeros(2)
    ckpt.check_master_free_load({0: {"exp_avg": z, "exp_avg_sq": z, "step": 3}})
    for name in ("master_residual", "master_param"):
        with pytest.raises(ValueError, match=name):
            ckpt.check_master_free_load({0: {"exp_avg": z}, 1: {name: z}})

