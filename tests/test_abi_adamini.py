"""The fused Adam-mini's C ABI and host logic without a GPU: the symbols, the argument checks that
come before any upload or launch, ``optimizer_kind``, the constructors' refusals, the layout of the
block state and the class's own checks."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from test_abi_adafactor import _refused

NAMES = ("zs_adamini_hparams_init", "zs_adaminiset_create", "zs_adaminiset_run",
         "zs_adaminiset_run_pass", "zs_adaminiset_stats", "zs_adaminiset_destroy")


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    integration = (REPO / "INTEGRATION.md").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert name in _lib.EXPORTED and name in _lib._SIGS and hasattr(so, name)
        assert re.search(rf"^int {name}\(", text, re.M) and name in integration
    assert re.search(r"^} zs_adamini_seg;$", text, re.M) and re.search(r"^} zs_adamini_hparams;$", text, re.M)
    assert re.search(r"^#define ZS_ABI_VERSION 13$", text, re.M)
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    code = _lib.LIB_PATH.read_bytes()  # the kernels are in the code object
    assert all(k in code for k in (b"adamini_resident_kernel", b"adamini_partial_kernel",
                                   b"adamini_finish_kernel", b"adamini_apply_kernel"))
    assert ctypes.sizeof(_lib.AdamMiniSeg) == 80 and ctypes.sizeof(_lib.AdamMiniHParams) == 56


def test_hparams_init_validates_like_the_class():
    from zero_amd.kernels import adamini_hparams as hp

    for kw, word in ((dict(lr=-1.0), "learning rate"), (dict(lr=float("nan")), "learning rate"),
                     (dict(beta1=1.0), "index 0"), (dict(beta2=-0.1), "index 1"), (dict(eps=-1e-8), "epsilon"),
                     (dict(weight_decay=-0.1), "weight_decay"), (dict(grad_div=0.0), "grad_div")):
        _refused(lambda: hp(**kw), "zs_adamini_hparams_init", word)
    h = hp()
    assert (h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.grad_div, h.maximize) == \
        (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0)


def test_create_and_run_refuse_without_a_device():
    """Host addresses stand in for device ones: every call returns before an upload or a launch."""
    from zero_amd import _lib
    from zero_amd.kernels import (AdafactorSet, AdamMiniSet, MuonSet, adafactor_hparams, adam_hparams,
                                  adamini_hparams, muon_hparams)

    BF16, SPLIT = _lib.ZS_BF16, _lib.ZS_BF16_SPLIT
    a = 1 << 20

    def row(**k):
        r = dict(g=a, master=a, master_out=a, p_out=0, m=a, v=a, R=4, C=8, block_rows=1, param=0)
        r.update(k)
        return [r[f] for f in AdamMiniSet.FIELDS]

    make = lambda rows, g=BF16, p=BF16, **kw: AdamMiniSet(np.array(rows, np.uint64), g, p, **kw)  # noqa: E731
    for args, kw, word in ((([], 7), {}, "g_dtype"), (([], BF16, _lib.ZS_BF16_SR), {}, "p_dtype"),
                           (([],), dict(resident_cap=16385), "resident_cap"),
                           (([row(g=0)],), {}, "missing"), (([row(m=0)],), {}, "missing"),
                           (([row(v=0)],), {}, "missing"), (([row(R=0)],), {}, "R and C"),
                           (([row(block_rows=3)],), {}, "does not divide"),
                           (([row(master_out=a + 64)],), {}, "in place"),
                           (([row()], BF16, SPLIT), {}, "split master needs p_out"),
                           (([row(g=a + 1)],), {}, "aligned"), (([row(v=a + 2)],), {}, "aligned")):
        _refused(lambda: make(*args, **kw), "zs_adaminiset_create", word)
    lib, R = _lib.lib, ctypes.byref
    hp, ahp = adamini_hparams(), adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    empty = make([])
    assert (empty.elems, empty.bytes, empty.scratch_bytes, empty.blocks) == (0, 0, 0, 0)
    adam = ctypes.c_void_p()
    _lib.call("zs_adamset_create", None, 0, BF16, SPLIT, R(adam))
    af, mu = AdafactorSet(np.zeros((0, 9), np.uint64), BF16), MuonSet(np.zeros((0, 8), np.uint64), BF16)
    try:
        for args, text in (((None, R(hp), 1, 0), b"NULL"), ((empty._h, None, 1, 0), b"NULL"),
                           ((empty._h, R(hp), 0, 0), b"step must be >= 1"),
                           ((adam, R(hp), 1, 0), b"zs_adaminiset_create"),
                           ((af._h, R(hp), 1, 0), b"zs_adaminiset_create"),
                           ((mu._h, R(hp), 1, 0), b"zs_adaminiset_create")):
            assert lib.zs_adaminiset_run(*args) == _lib.ZS_ERR_INVALID, args
            msg = lib.zs_last_error()
            assert msg.startswith(b"zs_adaminiset_run:") and text in msg, msg
        # the other families' entry points refuse an Adam-mini set
        for name, args in (("zs_adamset_run", (empty._h, R(ahp), 0)),
                           ("zs_adafactorset_run", (empty._h, R(adafactor_hparams()), 1, 0)),
                           ("zs_muonset_run", (empty._h, R(muon_hparams()), 0))):
            assert getattr(lib, name)(*args) == _lib.ZS_ERR_INVALID, name
            assert lib.zs_last_error().startswith(name.encode() + b":")
        empty.run(hp, 1, 0)  # an empty set has nothing to launch
        empty.run_pass(hp, 7, 2, 0)
        _refused(lambda: empty.run_pass(hp, 1, 3, 0), "pass")
        hp.beta2 = 1.0  # a struct filled by hand gets the same rules
        _refused(lambda: empty.run(hp, 1, 0), "zs_adaminiset_run", "index 1")
    finally:
        lib.zs_adamset_destroy(adam)


def _adamini(dtype=torch.float32, **kw):
    from zero_amd.optim import AdamMini

    return AdamMini([torch.nn.Parameter(torch.zeros(8, 4, dtype=dtype))], **kw)


def test_optimizer_kind_and_group_hparams():
    from zero_amd._sharded import group_hparams, optimizer_kind
    from zero_amd._update import KIND_NAMES, KINDS

    assert optimizer_kind(_adamini()) == "adamini" and "adamini" in KINDS and "AdamMini" in KIND_NAMES["adamini"]
    with pytest.raises(TypeError, match=r"Adafactor.*Lion.*NorMuon.*AdamMini.*RMSprop"):
        optimizer_kind(torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(2))]))
    opt = _adamini(lr=torch.tensor(0.5), betas=(0.8, 0.9), eps=1e-6, weight_decay=0.1, block_rows=2,
                   maximize=True)
    assert group_hparams("adamini", opt.param_groups[0], opt) == dict(
        lr=0.5, beta1=0.8, beta2=0.9, eps=1e-6, weight_decay=0.1, block_rows=2, maximize=True,
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

    with pytest.raises(ValueError, match=rf"AdamMini.*{list(kw)[-1]}"):
        zero2.ShardedOptimizer(_adamini(torch.bfloat16 if "master" in kw else torch.float32), **kw)


def test_zero1_and_zero3_constructors_refuse(monkeypatch):
    from zero_amd import _sharded, zero1, zero3

    for update in (False, True):
        with pytest.raises(ValueError, match="AdamMini.*ZeRO-3"):
            zero3.ShardedOptimizer(_adamini(), update=update)
    world = {"ws": 2, "rank": 0}
    monkeypatch.setattr(_sharded, "get", lambda what, dm=None: world[what])
    with pytest.raises(ValueError, match="AdamMini.*ZeRO-1 at world size > 1"):
        zero1.ShardedOptimizer(_adamini())


def test_state_layout_and_the_class():
    from zero_amd._update import state_layout
    from zero_amd.flat import AdamMiniState as S
    from zero_amd.optim import AdamMini

    assert state_layout("adamini", 1001) == (1001, {"m": (0, torch.float32)})  # exp_avg alone
    assert (S.blocks((37, 53), 1), S.blocks((64, 8), 16), S.blocks((4, 9, 16), 2), S.blocks((6, 5), 0),
            S.blocks((1000,), 7), S.blocks((), 1)) == (37, 4, 2, 1, 1, 1)
    with pytest.raises(ValueError, match="block_rows=3 does not divide the 8 rows"):
        _adamini(block_rows=3)
    w, b = torch.nn.Parameter(torch.ones(6, 4)), torch.nn.Parameter(torch.ones(10))
    opt = AdamMini([w, b], lr=0.1, block_rows=3)
    w.grad, b.grad = torch.ones(6, 4), torch.arange(10.0)
    opt.step()
    assert opt.state[w]["block_exp_avg_sq"].shape == (2,) and opt.state[b]["block_exp_avg_sq"].shape == (1,)
    assert float(opt.state[b]["step"]) == 1 and torch.allclose(w, torch.full((6, 4), 0.9), atol=1e-6)
    assert torch.allclose(opt.state[b]["block_exp_avg_sq"], torch.tensor([28.5e-3]))  # mean k^2 = 28.5
