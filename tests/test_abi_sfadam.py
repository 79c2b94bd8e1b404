"""The fused Schedule-Free AdamW's C ABI and host logic without a GPU (nothing is launched)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import REPO

NAMES = ("zs_sfadam_hparams_init", "zs_sfadamset_create", "zs_sfadamset_run", "zs_sfadamset_swap")


def _class(dtype=torch.float32, **kw):
    from zero_amd.optim import ScheduleFreeAdamW

    return ScheduleFreeAdamW([torch.nn.Parameter(torch.zeros(8, dtype=dtype))], **kw)


def test_symbols_and_the_order_of_the_kinds():
    from zero_amd import _lib
    from zero_amd._sharded import optimizer_kind
    from zero_amd._update import KINDS

    text = (REPO / "include" / "zero_amd.h").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert re.search(rf"^int {name}\(", text, re.M), name
        assert name in _lib.EXPORTED and name in _lib._SIGS and hasattr(so, name)
        assert name in (REPO / "INTEGRATION.md").read_text()
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    assert optimizer_kind(_class()) == "sfadam" and KINDS[-1] == "sfadam"
    assert KINDS[:9] == ("adam", "sgd", "lion", "adafactor", "muon", "lamb", "normuon", "adamini",
                         "apollo")
    for old in (r"Lion.*RMSprop", r"Adafactor.*Lion.*RMSprop",
                r"Adafactor.*Lion.*NorMuon.*AdamMini.*Apollo.*ScheduleFreeAdamW.*RMSprop"):
        with pytest.raises(TypeError, match=old):
            optimizer_kind(torch.optim.RMSprop([torch.nn.Parameter(torch.zeros(2))]))


@pytest.mark.parametrize("word,bad", [
    ("learning rate", dict(lr=-1e-3)), ("beta1", dict(betas=(0.0, 0.999))),
    ("beta1", dict(betas=(1.0, 0.999))), ("beta2", dict(betas=(0.9, 1.0))),
    ("epsilon", dict(eps=-1e-8)), ("weight_decay", dict(weight_decay=-1e-2))])
def test_hparams_init_and_the_class_refuse_the_same(word, bad):
    from zero_amd import _lib
    from zero_amd.kernels import sfadam_hparams

    with pytest.raises(ValueError):
        _class(**bad)
    with pytest.raises(ValueError):  # (the warm-up is the host's: the init never sees it)
        _class(warmup_steps=-1)
    kw = dict(dict(lr=2.5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), **bad)
    with pytest.raises(_lib.ZeroAmdError, match=word):
        sfadam_hparams(kw["lr"], *kw["betas"], kw["eps"], kw["weight_decay"])


def test_create_run_and_swap_refuse_before_any_device_work():
    """Bad tables, foreign sets and bad arguments raise ZS_ERR_INVALID with their message before
    anything is uploaded or launched (host addresses stand in, never read); an empty set runs."""
    from zero_amd import _lib
    from zero_amd.kernels import (AdamSet, LionSet, SfAdamSet, SgdSet, adam_hparams, lion_hparams,
                                  sfadam_hparams, sgd_hparams)

    F32, BF16, SPLIT, SR = _lib.ZS_F32, _lib.ZS_BF16, _lib.ZS_BF16_SPLIT, _lib.ZS_BF16_SR
    a = 1 << 20  # a 16-byte aligned address; nothing dereferences it

    def row(**k):
        return [list(dict(dict(g=a, master=a, master_out=a, p_out=0, m=a, v=a, vmax=0, carry=0,
                               n=8), **k).values())]

    none = np.zeros((0, 9), np.uint64)
    hp, bad_c = sfadam_hparams(1e-3), sfadam_hparams(1e-3)
    bad_c.c = 2.0
    sf, others = SfAdamSet(none, BF16, SPLIT), [C(none, BF16, SPLIT) for C in (AdamSet, SgdSet, LionSet)]
    cases = [(lambda: SfAdamSet(none, 7, BF16), "g_dtype"),
             (lambda: SfAdamSet(none, BF16, SR), "p_dtype"),
             (lambda: SfAdamSet(row(m=0), F32, BF16), "missing master/m/v"),
             (lambda: SfAdamSet(row(vmax=a), F32, BF16), "vmax must be 0"),
             (lambda: SfAdamSet(row(master_out=0), BF16, SPLIT), "split master"),
             (lambda: SfAdamSet(row(carry=a) + row(), F32, BF16), "all segments or none"),
             (lambda: sf.run(hp, 0, guard=True), "guard"), (lambda: sf.run(bad_c, 0), "c must lie"),
             (lambda: sf.swap(float("nan"), True, 0), "finite"),
             # the other families' entry points refuse a Schedule-Free set ...
             (lambda: AdamSet.run(sf, adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1), 0), "zs_sfadamset_create"),
             (lambda: SgdSet.run(sf, sgd_hparams(0.1), 0), "zs_sfadamset_create"),
             (lambda: LionSet.run(sf, lion_hparams(1e-4), 0), "zs_lionset_create")]
    for other in others:  # ... and it refuses their sets
        cases += [(lambda o=other: SfAdamSet.run(o, hp, 0), "zs_sfadamset_create"),
                  (lambda o=other: SfAdamSet.swap(o, 0.1, True, 0), "zs_sfadamset_create")]
    for call, text in cases:
        with pytest.raises(_lib.ZeroAmdError, match=text) as e:
            call()
        assert e.value.code == _lib.ZS_ERR_INVALID
    sf.run(hp, 0)  # an empty set has nothing to launch
    sf.swap(1 - 1 / 0.9, True, 0)
    sf.swap(0.1, False, 0)


@pytest.mark.parametrize("kw", [
    dict(max_grad_norm=1.0, skip_nonfinite=True), dict(state_dtype=torch.bfloat16),
    dict(state_rounding="stochastic"), dict(master="none"), dict(ema_decay=0.9),
    dict(param_update_norms=True)], ids=lambda kw: next(iter(reversed(kw))))
def test_constructors_refuse_before_any_device_work(kw, monkeypatch):
    """CPU parameters, no process group (ZeRO-1 asks for the world size first: it is told 1)."""
    from zero_amd import _sharded, zero1, zero2, zero3

    monkeypatch.setattr(_sharded, "get", lambda what, dm=None: {"ws": 1, "rank": 0}[what])
    dt = torch.bfloat16 if kw.get("master") == "none" else torch.float32
    for make in (zero1.ShardedOptimizer, zero2.ShardedOptimizer,
                 lambda o, **k: zero3.ShardedOptimizer(o, update=True, **k)):
        with pytest.raises(ValueError, match="ScheduleFreeAdamW"):
            make(_class(dt), **kw)
    with pytest.raises(ValueError, match="ScheduleFreeAdamW.*arena='buckets'"):
        zero2.ShardedOptimizer(_class(), arena="buckets")
    with pytest.raises(ValueError, match="ScheduleFreeAdamW.*reference mode"):
        zero3.ShardedOptimizer(_class(), update=False)
