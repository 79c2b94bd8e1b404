"""The sharded EMA's C ABI and host logic without a GPU: the symbol, its argument checks (nothing is
launched for any of them), ``check_ema_decay``, the optimizers' refusals before any device work, and
``ema_param`` in the state views and checkpoint entries of the update core on CPU tensors.  (The two
refusals that need a set with segments -- the carry and a missing vmax column -- are in
tests/test_gpu_adam_ema.py: a table with segments is uploaded to the device.)"""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import REPO

NAME = "zs_adamset_run_ema"


def test_symbol_is_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    assert re.search(r"^int %s\(const zs_adamset\* as, const zs_adam_hparams\* hp, "
                     r"const float\* coef, int guard,\s+float ema_weight, uintptr_t stream\);" % NAME,
                     text, re.M)
    assert NAME in _lib.EXPORTED and NAME in _lib._SIGS and hasattr(so, NAME)
    assert NAME in (REPO / "INTEGRATION.md").read_text()
    assert re.search(r"^#define ZS_ABI_VERSION 13$", text, re.M)
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    assert b"AdamEmaRule" in _lib.LIB_PATH.read_bytes()  # the instances are in the code object


def _empty_set(create, *args):
    from zero_amd import _lib

    h = ctypes.c_void_p()
    _lib.call(create, None, 0, *args, ctypes.byref(h))  # no segments: nothing is uploaded
    return h


def test_argument_checks_launch_nothing():
    from zero_amd import _lib

    lib = _lib.lib
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data  # a host address: every call below returns before a launch
    hp, ams = _lib.AdamHParams(), _lib.AdamHParams()
    ams.amsgrad = 1
    plain = _empty_set("zs_adamset_create", _lib.ZS_BF16, _lib.ZS_BF16_SPLIT)
    sgd = _empty_set("zs_sgdset_create", _lib.ZS_BF16, _lib.ZS_BF16_SPLIT)
    bf16_state = _empty_set("zs_adamset_create_ex", _lib.ZS_BF16, _lib.ZS_BF16_SPLIT, _lib.ZS_BF16)
    psr = _empty_set("zs_adamset_create_ex", _lib.ZS_BF16, _lib.ZS_BF16_SR, _lib.ZS_F32)
    f = ctypes.c_float
    try:
        cases = (
            ((None, ctypes.byref(hp), p, 0, f(0.5), 0), b"NULL"),
            ((plain, None, p, 0, f(0.5), 0), b"NULL"),
            ((sgd, ctypes.byref(hp), p, 0, f(0.5), 0), b"zs_sgdset_create"),
            ((bf16_state, ctypes.byref(hp), p, 0, f(0.5), 0), b"ZS_BF16 state"),
            ((psr, ctypes.byref(hp), p, 0, f(0.5), 0), b"ZS_BF16_SR"),
            ((plain, ctypes.byref(ams), p, 0, f(0.5), 0), b"amsgrad"),
            ((plain, ctypes.byref(hp), None, 1, f(0.5), 0), b"guard"),
            ((plain, ctypes.byref(hp), p, 0, f(float("nan")), 0), b"ema_weight"),
            ((plain, ctypes.byref(hp), p, 0, f(-0.001), 0), b"ema_weight"),
            ((plain, ctypes.byref(hp), p, 0, f(1.001), 0), b"ema_weight"),
            ((plain, ctypes.byref(hp), None, 0, f(float("inf")), 0), b"ema_weight"),
        )
        for args, text in cases:
            assert getattr(lib, NAME)(*args) == _lib.ZS_ERR_INVALID, args
            msg = lib.zs_last_error()
            assert msg.startswith(NAME.encode() + b":") and text in msg, msg
        # the ends of the range are weights; an empty set has nothing to launch
        for w in (0.0, 1.0, 0.5):
            assert getattr(lib, NAME)(plain, ctypes.byref(hp), None, 0, f(w), 0) == _lib.ZS_OK
    finally:
        for h in (plain, sgd, bf16_state, psr):
            lib.zs_adamset_destroy(h)
    assert not buf.any()


def test_check_ema_decay():
    from zero_amd._update import check_ema_decay, ema_weight

    assert check_ema_decay(None) is None
    for good in (0, 1, 0.0, 1.0, 0.5, 0.999, np.float32(0.25), np.float64(0.9999)):
        assert check_ema_decay(good) == float(good)
    for bad in (-1e-9, 1.0000001, float("nan"), float("inf"), True, False, "0.9", [0.9]):
        with pytest.raises(ValueError, match="ema_decay"):
            check_ema_decay(bad)
    for d in (0.999, 0.9999, 0.99, 0.9, 0.5, 0.3, 0.0, 1.0):
        w = ema_weight(d)
        assert isinstance(w, float) and np.float32(w) == np.float32(1.0 - d) and w == float(np.float32(w))
    with pytest.raises(ValueError, match="ema_decay"):
        ema_weight(1.5)


def _adam(**kw):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(8))], lr=1e-3, **kw)


def _bf16_adam(**kw):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))], lr=1e-3, **kw)


def _sgd():
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(8))], lr=1e-3, momentum=0.9)


def test_zero2_constructor_refuses_before_any_device_work():
    """CPU parameters, no process group: each error below comes before the first thing that would
    need either."""
    from zero_amd import zero2

    for bad in (-0.1, 1.5, float("nan"), True, "0.9"):
        with pytest.raises(ValueError, match="ema_decay"):
            zero2.ShardedOptimizer(_adam(), ema_decay=bad)
    with pytest.raises(ValueError, match="SGD"):
        zero2.ShardedOptimizer(_sgd(), ema_decay=0.9)
    with pytest.raises(ValueError, match="amsgrad"):
        zero2.ShardedOptimizer(_adam(amsgrad=True), ema_decay=0.9)
    with pytest.raises(ValueError, match="ema_decay.*bfloat16"):
        zero2.ShardedOptimizer(_bf16_adam(betas=(0.9, 0.99)), ema_decay=0.9,
                               state_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="ema_decay.*master='none'"):
        zero2.ShardedOptimizer(_bf16_adam(), ema_decay=0.9, master="none")
    with pytest.raises(ValueError, match="ema_decay.*bucket arena"):
        zero2.ShardedOptimizer(_adam(), ema_decay=0.9, arena="buckets")
    with pytest.raises(ValueError, match="ema_decay.*overlap"):
        zero2.ShardedOptimizer(_adam(), ema_decay=0.9, overlap=True)


def test_zero1_constructor_refuses_before_any_device_work(monkeypatch):
    """ZeRO-1 asks for the world size first (its carry): answered here without a process group."""
    from zero_amd import _sharded, zero1

    world = {"ws": 2, "rank": 0}
    monkeypatch.setattr(_sharded, "get", lambda what, dm=None: world[what])
    with pytest.raises(ValueError, match="ema_decay.*ZeRO-1 at world size > 1"):
        zero1.ShardedOptimizer(_adam(), ema_decay=0.9)
    world["ws"] = 1
    with pytest.raises(ValueError, match="SGD"):
        zero1.ShardedOptimizer(_sgd(), ema_decay=0.9)
    with pytest.raises(ValueError, match="amsgrad"):
        zero1.ShardedOptimizer(_adam(amsgrad=True), ema_decay=0.9)
    with pytest.raises(ValueError, match="ema_decay.*bucket arena"):
        zero1.ShardedOptimizer(_adam(), ema_decay=0.9, layout="flat")  # (ZeRO-1: the bucket arena)
    with pytest.raises(ValueError, match="ema_decay.*overlap"):
        zero1.ShardedOptimizer(_adam(), ema_decay=0.9, overlap=True)


def test_zero3_constructor_refuses_before_any_device_work():
    from zero_amd import zero3

    with pytest.raises(ValueError, match="ema_decay.*update mode"):
        zero3.ShardedOptimizer(_adam(), update=False, ema_decay=0.9)
    for bad in (-0.1, 1.5, float("nan"), True):
        with pytest.raises(ValueError, match="ema_decay"):
            zero3.ShardedOptimizer(_adam(), update=True, ema_decay=bad)
    with pytest.raises(ValueError, match="SGD"):
        zero3.ShardedOptimizer(_sgd(), update=True, ema_decay=0.9)
    with pytest.raises(ValueError, match="amsgrad"):
        zero3.ShardedOptimizer(_adam(amsgrad=True), update=True, ema_decay=0.9)
    with pytest.raises(ValueError, match="ema_decay.*bfloat16"):
        zero3.ShardedOptimizer(_bf16_adam(betas=(0.9, 0.99)), update=True, ema_decay=0.9,
                               state_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="ema_decay.*master='none'"):
        zero3.ShardedOptimizer(_bf16_adam(), update=True, ema_decay=0.9, master="none")


# ---- the update core's views and checkpoint entries, on CPU tensors -------------------------------
def _core(L, *, split=False, fp32_master=False, ema=True):
    """An UpdateCore over CPU tensors (its constructor allocates on the device)."""
    from zero_amd._update import UpdateCore, state_layout

    core = UpdateCore.__new__(UpdateCore)
    core.kind, core.L = "adam", L
    total, lay = state_layout("adam", L, split=split, fp32_master=fp32_master)
    assert "ema" not in lay  # the EMA is an array of its own, like max_exp_avg_sq
    core.state = torch.zeros(total)
    for name in ("m", "v", "carry", "master", "lo"):
        off, dt = lay.get(name, (0, None))
        setattr(core, name, None if dt is None else core.state[off:].view(dt)[:L])
    core.vmax = None
    core.ema = torch.zeros(L) if ema else None
    core.master_free, core.state_dtype = False, torch.float32
    core.steps = np.zeros(1, np.int64)
    return core


def test_views_and_amsgrad_exclusion():
    core = _core(12)
    v = core.views(2, 6, (2, 3))
    assert list(v) == ["exp_avg", "exp_avg_sq", "ema_param"]
    assert v["ema_param"].shape == (2, 3) and v["ema_param"].dtype == torch.float32
    v["ema_param"].fill_(3.0)  # live: a view of the core's array
    assert core.ema[2:8].eq(3.0).all() and core.ema[:2].eq(0).all() and core.ema[8:].eq(0).all()
    with pytest.raises(ValueError, match="amsgrad"):
        core.ensure_vmax()
    assert "ema_param" not in _core(12, ema=False).views(0, 12, (12,))
    rows = np.zeros((2, 9), np.uint64)
    core.state_cols(rows, [0, 4])
    assert rows[0, 6] == core.ema.data_ptr() and rows[1, 6] == core.ema.data_ptr() + 16


@pytest.mark.parametrize("master", ["fp32-param", "fp32-master", "split"])
def test_save_and_load_entries(master):
    from zero_amd._update import join_split_master

    n = 6
    core = _core(n, split=master == "split", fp32_master=master == "fp32-master")
    g = torch.Generator().manual_seed(1)
    param = torch.randn(n, generator=g)
    if master != "fp32-param":
        param = param.to(torch.bfloat16)
    views = core.views(0, n, (n,))
    for t in views.values():
        if t.dtype == torch.int16:
            t.copy_(torch.randint(-30000, 30000, (n,), generator=g).to(torch.int16))
        else:
            t.copy_(torch.randn(n, generator=g))
    core.steps[0] = 5
    entry = core.save_entry(0, views, {})
    assert "ema_param" in entry and torch.equal(entry["ema_param"], views["ema_param"])
    assert entry["ema_param"].data_ptr() != views["ema_param"].data_ptr()  # a copy
    # with ema_param: restored bit for bit
    fresh = _core(n, split=master == "split", fp32_master=master == "fp32-master")
    fv = fresh.views(0, n, (n,))
    fresh.load_entry(0, fv, entry, param)
    for k in views:
        assert torch.equal(fv[k], views[k]), k
    assert fresh.steps[0] == 5
    # without: the EMA starts from the loaded master
    lean = {k: v for k, v in entry.items() if k != "ema_param"}
    fresh = _core(n, split=master == "split", fp32_master=master == "fp32-master")
    fv = fresh.views(0, n, (n,))
    fresh.load_entry(0, fv, lean, param)
    if master == "fp32-param":
        want = param
    elif master == "fp32-master":
        want = views["master_param"]
    else:
        want = join_split_master(param, views["master_residual"])
        hi = param.view(torch.int16).to(torch.int32).numpy().astype(np.int64) << 16
        bits = (hi + views["master_residual"].numpy().astype(np.int64)) & 0xFFFFFFFF
        assert np.array_equal(want.numpy().view(np.uint32), bits.astype(np.uint32))
    assert np.array_equal(fv["ema_param"].numpy().view(np.uint32),
                          want.float().numpy().view(np.uint32))
    # an entry with nothing at all (a parameter that never stepped): the EMA is the parameter
    fresh = _core(n, split=master == "split", fp32_master=master == "fp32-master")
    fv = fresh.views(0, n, (n,))
    fresh.load_entry(0, fv, {}, param)
    assert torch.equal(fv["ema_param"], param.float())


def test_loader_refuses_ema_entries_without_ema_decay():
    from zero_amd import checkpoint as ckpt

    ckpt.check_ema_load({})
    ckpt.check_ema_load({0: {"exp_avg": torch.zeros(2)}, 1: {}})
    with pytest.raises(ValueError, match="ema_param"):
        ckpt.check_ema_load({0: {"exp_avg": torch.zeros(2)}, 1: {"ema_param": torch.zeros(2)}})
