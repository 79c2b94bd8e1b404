"""The fused Adafactor's C ABI and host logic without a GPU: the symbols, the argument checks that
come before any upload or launch, ``optimizer_kind``, the constructors' refusals and the layout of
the factored state."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import REPO

NAMES = ("zs_adafactor_hparams_init", "zs_adafactorset_create", "zs_adafactorset_run",
         "zs_adafactorset_run_pass", "zs_adafactorset_stats", "zs_adafactorset_destroy")


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    integration = (REPO / "INTEGRATION.md").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert name in _lib.EXPORTED and name in _lib._SIGS and hasattr(so, name)
        assert re.search(rf"^int {name}\(", text, re.M) and name in integration
    assert re.search(r"^} zs_adafactor_seg;$", text, re.M) and re.search(r"^} zs_adafactor_hparams;$", text, re.M)
    assert re.search(r"^#define ZS_ABI_VERSION 13$", text, re.M)
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    assert b"adafactor_pass_kernel" in _lib.LIB_PATH.read_bytes()  # the kernels are in the code object
    assert ctypes.sizeof(_lib.AdafactorSeg) == 72 and ctypes.sizeof(_lib.AdafactorHParams) == 64


def _refused(fn, *words):
    from zero_amd import _lib

    with pytest.raises(_lib.ZeroAmdError) as e:
        fn()
    assert e.value.code == _lib.ZS_ERR_INVALID
    assert all(w in str(e.value) for w in words), str(e.value)


def test_hparams_init_validates_like_torch():
    from zero_amd.kernels import adafactor_hparams as hp

    for kw, word in ((dict(lr=0.0), "learning rate"), (dict(lr=float("nan")), "learning rate"),
                     (dict(beta2_decay=0.1), "beta2_decay"), (dict(eps=(-1e-30, 1e-3)), "epsilon1"),
                     (dict(eps=(None, 0.0)), "epsilon2"), (dict(d=0.5), "d should be >= 1"),
                     (dict(weight_decay=-0.1), "weight_decay"), (dict(grad_div=0.0), "grad_div")):
        _refused(lambda: hp(**kw), word)
    h = hp()
    assert (h.lr, h.beta2_decay, h.eps1, h.eps2, h.d, h.weight_decay, h.grad_div, h.maximize) == \
        (1e-2, -0.8, 2.0 ** -23, 1e-3, 1.0, 0.0, 1.0, 0)


def test_create_and_run_refuse_without_a_device():
    """Host addresses stand in for device ones: every call returns before an upload or a launch."""
    from zero_amd import _lib
    from zero_amd.kernels import AdafactorSet, adafactor_hparams, adam_hparams, lion_hparams, sgd_hparams

    BF16, SPLIT = _lib.ZS_BF16, _lib.ZS_BF16_SPLIT
    a = 1 << 20

    def row(**k):
        r = dict(g=a, master=a, master_out=a, p_out=0, row_var=a, col_var=a, R=4, C=8, param=0)
        r.update(k)
        return [r[f] for f in AdafactorSet.FIELDS]

    make = lambda rows, g=BF16, p=BF16: AdafactorSet(np.array(rows, np.uint64), g, p)  # noqa: E731
    for args, word in ((([], 7), "g_dtype"), (([], BF16, _lib.ZS_BF16_SR), "p_dtype"),
                       (([row(g=0)],), "missing"), (([row(row_var=0)],), "missing"),
                       (([row(R=0)],), "R and C"), (([row(col_var=0)],), "1-D entry"),
                       (([row(master_out=a + 64)],), "in place"),
                       (([row()], BF16, SPLIT), "split master needs p_out"),
                       (([row(g=a + 1)],), "aligned"),
                       (([row(), row(param=1), row()],), "not adjacent")):
        _refused(lambda: make(*args), word)
    lib, R = _lib.lib, ctypes.byref
    hp, ahp, shp, lhp = adafactor_hparams(), adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1), sgd_hparams(0.1), lion_hparams(1e-4)
    empty = make([])
    others = {}
    for name in ("zs_adamset_create", "zs_sgdset_create"):
        others[name] = ctypes.c_void_p()
        _lib.call(name, None, 0, BF16, SPLIT, R(others[name]))
    try:
        for args, text in (((None, R(hp), 1, 0), b"NULL"), ((empty._h, None, 1, 0), b"NULL"),
                           ((empty._h, R(hp), 0, 0), b"step must be >= 1"),
                           ((others["zs_adamset_create"], R(hp), 1, 0), b"zs_adafactorset_create"),
                           ((others["zs_sgdset_create"], R(hp), 1, 0), b"zs_adafactorset_create")):
            assert lib.zs_adafactorset_run(*args) == _lib.ZS_ERR_INVALID, args
            msg = lib.zs_last_error()
            assert msg.startswith(b"zs_adafactorset_run:") and text in msg, msg
        # the other families' entry points refuse an Adafactor set
        for name, args in (("zs_adamset_run", (empty._h, R(ahp), 0)),
                           ("zs_adamset_run_clipped", (empty._h, R(ahp), a, 0)),
                           ("zs_adamset_run_psr", (empty._h, R(ahp), None, 0, 0, 1, 2, 0)),
                           ("zs_adamset_run_ema", (empty._h, R(ahp), None, 0, ctypes.c_float(0.5), 0)),
                           ("zs_adamset_run_stats", (empty._h, R(ahp), None, 0, None, 0)),
                           ("zs_sgdset_run", (empty._h, R(shp), None, 0)),
                           ("zs_lionset_run", (empty._h, R(lhp), None, 0, 0, 0, 0, 0))):
            assert getattr(lib, name)(*args) == _lib.ZS_ERR_INVALID, name
            msg = lib.zs_last_error()
            assert msg.startswith(name.encode() + b":") and b"zs_adafactorset_create" in msg, msg
        empty.run(hp, 1, 0)  # an empty set has nothing to launch
        empty.run_pass(hp, 7, 2, 0)
    finally:
        for h in others.values():
            lib.zs_adamset_destroy(h)


def _adafactor(dtype=torch.float32, **kw):
    return torch.optim.Adafactor([torch.nn.Parameter(torch.zeros(8, 4, dtype=dtype))], **kw)


def test_optimizer_kind_and_group_hparams():
    from zero_amd._sharded import group_hparams, optimizer_kind

    assert optimizer_kind(_adafactor()) == "adafactor"
    with pytest.raises(TypeError, match=r"Adafactor.*Lion.*RMSprop"):
        optimizer_kind(torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(2))]))
    opt = _adafactor(lr=torch.tensor(0.5), beta2_decay=-0.7, eps=(1e-20, 1e-2), d=2.0,
                     weight_decay=0.1, maximize=True)
    assert group_hparams("adafactor", opt.param_groups[0], opt) == dict(
        lr=0.5, beta2_decay=-0.7, eps=(1e-20, 1e-2), d=2.0, weight_decay=0.1, maximize=True,
        amsgrad=False)


REFUSALS = [dict(layout="flat"), dict(arena="buckets"), dict(overlap=True), dict(grad_comm="bf16"),
            dict(max_grad_norm=1.0), dict(max_grad_norm=1.0, skip_nonfinite=True),
            dict(max_grad_norm=1.0, param_grad_norms=True), dict(state_dtype=torch.bfloat16),
            dict(state_rounding="nearest"), dict(master="none"), dict(ema_decay=0.9),
            dict(param_update_norms=True)]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: "-".join(kw))
def test_zero2_constructor_refuses_before_any_device_work(kw):
    """CPU parameters, no process group: the error comes before the first thing that needs either."""
    from zero_amd import zero2

    with pytest.raises(ValueError, match=rf"Adafactor.*{list(kw)[-1]}"):
        zero2.ShardedOptimizer(_adafactor(torch.bfloat16 if "master" in kw else torch.float32), **kw)


def test_zero1_and_zero3_constructors_refuse(monkeypatch):
    from zero_amd import _sharded, zero1, zero3

    for update in (False, True):
        with pytest.raises(ValueError, match="Adafactor.*ZeRO-3"):
            zero3.ShardedOptimizer(_adafactor(), update=update)
    world = {"ws": 2, "rank": 0}
    monkeypatch.setattr(_sharded, "get", lambda what, dm=None: world[what])
    with pytest.raises(ValueError, match="Adafactor.*ZeRO-1 at world size > 1"):
        zero1.ShardedOptimizer(_adafactor())


def test_state_layout():
    from zero_amd._update import state_layout
    from zero_amd.flat import AdafactorState as S

    assert state_layout("adafactor", 1001) == (0, {})  # the factors are an arena of their own
    assert state_layout("adafactor", 1001, split=True) == (501, {"lo": (0, torch.int16)})
    assert (S.sizes((37, 53)), S.sizes((2, 33, 40)), S.sizes((1000,)), S.sizes(())) == \
        ((37, 53), (66, 80), (1000,), (1,))
