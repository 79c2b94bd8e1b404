"""The fused Lion's C ABI and host logic without a GPU: the symbols, the argument checks of
zs_lion_hparams_init, zs_lionset_create and zs_lionset_run that need no device (nothing is launched
for any of them), ``state_layout("lion", ...)``, ``optimizer_kind`` and the optimizers' refusals
before any device work."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import REPO

NAMES = ("zs_lion_hparams_init", "zs_lionset_create", "zs_lionset_run")


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    assert re.search(r"^int zs_lion_hparams_init\(double lr, double beta1, double beta2, "
                     r"double weight_decay, int maximize,\s+double grad_div, double carry_mul, "
                     r"zs_lion_hparams\* hp\);", text, re.M)
    assert re.search(r"^int zs_lionset_create\(const zs_adam_seg\* segs, int64_t n, int g_dtype, "
                     r"int p_dtype,\s+int state_dtype, zs_adamset\*\* out\);", text, re.M)
    assert re.search(r"^int zs_lionset_run\(const zs_adamset\* as, const zs_lion_hparams\* hp, "
                     r"const float\* coef, int guard,\s+uint64_t m_base, uint32_t key0, "
                     r"uint32_t key1, uintptr_t stream\);", text, re.M)
    assert re.search(r"^} zs_lion_hparams;$", text, re.M)
    integration = (REPO / "INTEGRATION.md").read_text()
    for name in NAMES:
        assert name in _lib.EXPORTED and name in _lib._SIGS and hasattr(so, name)
        assert name in integration
    assert re.search(r"^#define ZS_ABI_VERSION 13$", text, re.M)
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    assert b"LionRuleT" in _lib.LIB_PATH.read_bytes()  # the instances are in the code object
    assert ctypes.sizeof(_lib.LionHParams) == 36


def _refused(fn, *words):
    from zero_amd import _lib

    with pytest.raises(_lib.ZeroAmdError) as e:
        fn()
    assert e.value.code == _lib.ZS_ERR_INVALID
    assert all(w in str(e.value) for w in words), str(e.value)


def test_hparams_init_refuses_what_lion_refuses():
    from zero_amd import _lib
    from zero_amd.kernels import lion_hparams

    _refused(lambda: lion_hparams(-1e-4), "learning rate")
    _refused(lambda: lion_hparams(1e-4, 1.0), "beta1")
    _refused(lambda: lion_hparams(1e-4, -0.1), "beta1")
    _refused(lambda: lion_hparams(1e-4, 0.9, 1.0), "beta2")
    _refused(lambda: lion_hparams(1e-4, 0.9, -0.5), "beta2")
    _refused(lambda: lion_hparams(1e-4, float("nan")), "beta1")
    _refused(lambda: lion_hparams(1e-4, weight_decay=-1e-2), "weight_decay")
    _refused(lambda: lion_hparams(1e-4, grad_div=0.0), "grad_div")
    _refused(lambda: lion_hparams(1e-4, grad_div=-2.0), "grad_div")
    _refused(lambda: _lib.call("zs_lion_hparams_init", 1e-4, 0.9, 0.99, 0.0, 0, 1.0, 0.0, None),
             "NULL")
    hp = lion_hparams(1e-4)
    assert hp.grad_div == 1.0 and hp.carry_mul == 0.0 and hp.maximize == 0


def _create(rows, g_dtype, p_dtype, state_dtype):
    from zero_amd import _lib

    rows = np.ascontiguousarray(np.asarray(rows, np.uint64).reshape(-1, 9))
    arr = (_lib.AdamSeg * max(len(rows), 1))()
    ctypes.memmove(arr, rows.ctypes.data, rows.nbytes)
    h = ctypes.c_void_p()
    _lib.call("zs_lionset_create", arr if len(rows) else None, len(rows), g_dtype, p_dtype,
              state_dtype, ctypes.byref(h))
    return h


def test_create_refuses_without_a_device():
    """Every refusal of zs_lionset_create comes before the tables are uploaded: host addresses
    (never read) stand in for device ones."""
    from zero_amd import _lib

    F32, BF16, SPLIT, SR = _lib.ZS_F32, _lib.ZS_BF16, _lib.ZS_BF16_SPLIT, _lib.ZS_BF16_SR
    a = 1 << 20  # a 16-byte aligned address; nothing dereferences it

    def row(**k):
        r = dict(g=a, master=a, master_out=a, p_out=0, m=a, v=0, vmax=0, carry=0, n=8)
        r.update(k)
        return [r[f] for f in ("g", "master", "master_out", "p_out", "m", "v", "vmax", "carry", "n")]

    _refused(lambda: _lib.call("zs_lionset_create", None, 0, F32, BF16, F32, None), "out is NULL")
    _refused(lambda: _create([], 7, BF16, F32), "g_dtype")
    _refused(lambda: _create([], F32, SR, F32), "p_dtype")
    _refused(lambda: _create([], F32, F32, F32), "p_dtype")
    _refused(lambda: _create([], F32, BF16, _lib.ZS_U8), "state_dtype")
    _refused(lambda: _create([row(m=0)], F32, BF16, F32), "missing master/m")
    _refused(lambda: _create([row(master=0)], F32, BF16, F32), "missing master/m")
    _refused(lambda: _create([row(v=a)], F32, BF16, F32), "v and vmax must be 0")
    _refused(lambda: _create([row(vmax=a)], F32, BF16, F32), "v and vmax must be 0")
    _refused(lambda: _create([row(n=(1 << 64) - 1)], F32, BF16, F32), "n < 0")  # int64 -1
    _refused(lambda: _create([row(master_out=0)], BF16, SPLIT, F32), "split master")
    _refused(lambda: _create([row(p_out=a, carry=a)], BF16, BF16, BF16), "ZS_BF16 state", "carry")
    _refused(lambda: _create([row(p_out=a, carry=a)], F32, SPLIT, F32), "fp32 grads", "carry")
    _refused(lambda: _create([row(carry=a), row()], F32, BF16, F32), "carry", "all segments or none")
    _refused(lambda: _lib.call("zs_lionset_create", None, 2, F32, BF16, F32,
                               ctypes.byref(ctypes.c_void_p())), "bad table")


def test_run_argument_checks_launch_nothing():
    from zero_amd import _lib

    lib = _lib.lib
    F32, BF16, SPLIT = _lib.ZS_F32, _lib.ZS_BF16, _lib.ZS_BF16_SPLIT
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data  # a host address: every call below returns before a launch
    from zero_amd.kernels import adam_hparams, lion_hparams, sgd_hparams

    hp, ahp, shp = lion_hparams(1e-4), adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1), sgd_hparams(0.1)
    lion = _create([], BF16, SPLIT, F32)
    lion16 = _create([], BF16, SPLIT, BF16)
    h = ctypes.c_void_p()
    _lib.call("zs_adamset_create", None, 0, BF16, SPLIT, ctypes.byref(h))
    adam = h
    h = ctypes.c_void_p()
    _lib.call("zs_sgdset_create", None, 0, BF16, SPLIT, ctypes.byref(h))
    sgd = h

    def hand(**k):
        x = _lib.LionHParams(neg_lr=-1e-4, beta1=0.9, one_minus_beta1=0.1, beta2=0.99,
                             one_minus_beta2=0.01, decay_mul=1.0, grad_div=1.0, carry_mul=0.0,
                             maximize=0)
        for name, val in k.items():
            setattr(x, name, val)
        return x

    R = ctypes.byref
    try:
        run = lib.zs_lionset_run
        cases = (
            ((None, R(hp), None, 0, 0, 0, 0, 0), b"NULL"),
            ((lion, None, None, 0, 0, 0, 0, 0), b"NULL"),
            ((adam, R(hp), None, 0, 0, 0, 0, 0), b"zs_lionset_create"),
            ((sgd, R(hp), None, 0, 0, 0, 0, 0), b"zs_lionset_create"),
            ((lion, R(hp), None, 1, 0, 0, 0, 0), b"guard"),
            ((lion, R(hand(neg_lr=1e-4)), None, 0, 0, 0, 0, 0), b"learning rate"),
            ((lion, R(hand(beta1=1.5)), None, 0, 0, 0, 0, 0), b"betas"),
            ((lion, R(hand(beta2=-0.5)), None, 0, 0, 0, 0, 0), b"betas"),
            ((lion, R(hand(grad_div=0.0)), None, 0, 0, 0, 0, 0), b"grad_div"),
        )
        for args, text in cases:
            assert run(*args) == _lib.ZS_ERR_INVALID, args
            msg = lib.zs_last_error()
            assert msg.startswith(b"zs_lionset_run:") and text in msg, msg
        # the other families' entry points refuse a Lion set
        s = 0
        others = (
            ("zs_adamset_run", (lion, R(ahp), s)),
            ("zs_adamset_run_clipped", (lion, R(ahp), p, s)),
            ("zs_adamset_run_guarded", (lion, R(ahp), p, s)),
            ("zs_adamset_run_sr", (lion16, R(ahp), None, 0, 1, 2, s)),
            ("zs_adamset_run_sr_guarded", (lion16, R(ahp), p, 0, 1, 2, s)),
            ("zs_adamset_run_psr", (lion16, R(ahp), None, 0, 0, 1, 2, s)),
            ("zs_adamset_run_ema", (lion, R(ahp), None, 0, ctypes.c_float(0.5), s)),
            ("zs_adamset_run_stats", (lion, R(ahp), None, 0, None, s)),
            ("zs_sgdset_run", (lion, R(shp), None, s)),
        )
        for name, args in others:
            assert getattr(lib, name)(*args) == _lib.ZS_ERR_INVALID, name
            msg = lib.zs_last_error()
            assert msg.startswith(name.encode() + b":"), msg
            assert b"zs_lionset_create" in msg or b"ZS_BF16_SR" in msg, msg
        # stochastic rounding is a bf16-momentum set's
        assert lib.zs_adamset_set_state_rounding(lion, 1) == _lib.ZS_ERR_INVALID
        assert lib.zs_adamset_set_state_rounding(lion16, 1) == _lib.ZS_OK
        # an empty set has nothing to launch: every valid form returns ZS_OK
        for aset in (lion, lion16):
            assert run(aset, R(hp), None, 0, 0, 0, 0, 0) == _lib.ZS_OK
            assert run(aset, R(hp), p, 0, 0, 0, 0, 0) == _lib.ZS_OK
            assert run(aset, R(hp), p, 1, 0, 1, 2, 0) == _lib.ZS_OK
        e, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert lib.zs_adamset_stats(lion, R(e), R(b)) == _lib.ZS_OK and (e.value, b.value) == (0, 0)
        n = ctypes.c_int64(-1)
        assert lib.zs_adamset_sqnorm_partials(lion, R(n)) == _lib.ZS_OK and n.value == 0
    finally:
        for x in (lion, lion16, adam, sgd):
            lib.zs_adamset_destroy(x)
    assert not buf.any()


def test_state_layout():
    from zero_amd._update import state_layout

    f32, bf16, i16 = torch.float32, torch.bfloat16, torch.int16
    L = 1001
    assert state_layout("lion", L) == (L, {"m": (0, f32)})
    assert state_layout("lion", L, momentum=False) == (L, {"m": (0, f32)})  # always one moment
    assert state_layout("lion", L, carry=True, fp32_master=True) == \
        (3 * L, {"m": (0, f32), "carry": (L, f32), "master": (2 * L, f32)})
    assert state_layout("lion", L, split=True) == (L + 501, {"m": (0, f32), "lo": (L, i16)})
    # bf16 momentum: L bf16 in 501 words, every later array at a multiple of 4 words (16 bytes)
    assert state_layout("lion", L, state_dtype=bf16) == (501, {"m": (0, bf16)})
    assert state_layout("lion", L, state_dtype=bf16, split=True) == \
        (504 + 501, {"m": (0, bf16), "lo": (504, i16)})
    assert state_layout("lion", L, state_dtype=bf16, fp32_master=True) == \
        (504 + L, {"m": (0, bf16), "master": (504, f32)})
    assert state_layout("lion", 8, state_dtype=bf16, split=True) == (8, {"m": (0, bf16), "lo": (4, i16)})
    with pytest.raises(ValueError, match="carry"):
        state_layout("lion", L, state_dtype=bf16, carry=True)
    with pytest.raises(ValueError, match="Lion"):
        state_layout("lion", L, master="none")
    # Adam's and SGD's layouts are what they were
    assert state_layout("adam", L, state_dtype=bf16, split=True) == \
        (504 + 501 + 3 + 501, {"m": (0, bf16), "v": (504, bf16), "lo": (1008, i16)})
    assert state_layout("sgd", L, momentum=False) == (0, {})


def _lion(dtype=torch.float32, **kw):
    from zero_amd.optim import Lion

    return Lion([torch.nn.Parameter(torch.zeros(8, dtype=dtype))], **kw)


def test_optimizer_kind():
    from zero_amd._sharded import group_hparams, optimizer_kind

    assert optimizer_kind(_lion()) == "lion"
    assert optimizer_kind(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(2))])) == "adam"
    assert optimizer_kind(torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1)) == "sgd"
    with pytest.raises(TypeError, match=r"Lion.*RMSprop"):
        optimizer_kind(torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(2))]))
    opt = _lion(lr=3e-4, betas=(0.95, 0.98), weight_decay=0.1, maximize=True)
    assert group_hparams("lion", opt.param_groups[0], opt) == dict(
        lr=3e-4, beta1=0.95, beta2=0.98, weight_decay=0.1, maximize=True, amsgrad=False)


def test_zero2_constructor_refuses_before_any_device_work():
    """CPU parameters, no process group: each error below comes before the first thing that would
    need either."""
    from zero_amd import zero2

    bf16 = torch.bfloat16
    with pytest.raises(ValueError, match="master='none'.*Lion"):
        zero2.ShardedOptimizer(_lion(bf16), master="none")
    with pytest.raises(ValueError, match="ema_decay.*Lion"):
        zero2.ShardedOptimizer(_lion(), ema_decay=0.9)
    with pytest.raises(ValueError, match="param_update_norms.*Lion"):
        zero2.ShardedOptimizer(_lion(), param_update_norms=True)
    with pytest.raises(ValueError, match="Lion.*arena='buckets'"):
        zero2.ShardedOptimizer(_lion(), arena="buckets")
    with pytest.raises(ValueError, match="Lion.*layout='zero'"):
        zero2.ShardedOptimizer(_lion(), layout="zero")
    with pytest.raises(ValueError, match="beta2 <= 0.99609375"):
        zero2.ShardedOptimizer(_lion(bf16, betas=(0.9, 0.999)), state_dtype=bf16)
    with pytest.raises(ValueError, match="stochastic.*bfloat16"):
        zero2.ShardedOptimizer(_lion(), state_rounding="stochastic")


def test_zero1_constructor_refuses_before_any_device_work(monkeypatch):
    from zero_amd import _sharded, zero1

    world = {"ws": 2, "rank": 0}
    monkeypatch.setattr(_sharded, "get", lambda what, dm=None: world[what])
    with pytest.raises(ValueError, match="bfloat16.*ZeRO-1 at world size > 1"):
        zero1.ShardedOptimizer(_lion(torch.bfloat16), state_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="Lion.*layout='flat'"):
        zero1.ShardedOptimizer(_lion(), layout="flat")  # (ZeRO-1: the bucket arena)
    with pytest.raises(ValueError, match="ema_decay"):
        zero1.ShardedOptimizer(_lion(), ema_decay=0.9)


def test_zero3_constructor_refuses_before_any_device_work():
    from zero_amd import zero3

    bf16 = torch.bfloat16
    with pytest.raises(ValueError, match="bfloat16.*update mode"):
        zero3.ShardedOptimizer(_lion(bf16), update=False, state_dtype=bf16)
    with pytest.raises(ValueError, match="master='none'.*Lion"):
        zero3.ShardedOptimizer(_lion(bf16), update=True, master="none")
    with pytest.raises(ValueError, match="ema_decay.*Lion"):
        zero3.ShardedOptimizer(_lion(), update=True, ema_decay=0.9)
    with pytest.raises(ValueError, match="param_update_norms.*Lion"):
        zero3.ShardedOptimizer(_lion(), update=True, param_update_norms=True)
    with pytest.raises(ValueError, match="beta2 <= 0.99609375"):
        zero3.ShardedOptimizer(_lion(bf16, betas=(0.9, 0.999)), update=True, state_dtype=bf16)
