"""The fused NorMuon's C ABI and its Python front without a GPU: the symbols, the checks that come
before any allocation or launch, and how ShardedOptimizer names the class."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from test_abi_muon import _refused

NAMES = ("zs_normuon_hparams_init", "zs_muonset_attach_rows", "zs_muonset_run_normuon",
         "zs_muonset_run_normuon_pass", "zs_muonset_rows")


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    integration = (REPO / "INTEGRATION.md").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert name in _lib.EXPORTED and name in _lib._SIGS and hasattr(so, name)
        assert re.search(rf"^int {name}\(", text, re.M) and name in integration
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    code = _lib.LIB_PATH.read_bytes()  # the kernels are in the code object
    assert all(k in code for k in (b"normuon_rowsq_kernel", b"normuon_finish_kernel", b"normuon_apply_kernel"))
    assert ctypes.sizeof(_lib.NorMuonHParams) == 96


def test_hparams_and_runs_refuse_without_a_device():
    from zero_amd import _lib
    from zero_amd.kernels import MuonSet, normuon_hparams

    for kw, word in ((dict(ns_steps=100), "Newton-Schulz"), (dict(lr=-1.0), "learning rate"),
                     (dict(momentum=-0.1), "momentum"), (dict(weight_decay=-0.1), "weight decay"),
                     (dict(grad_div=0.0), "grad_div"), (dict(beta2=1.0), "beta2"),
                     (dict(beta2=-0.1), "beta2"), (dict(norm_eps=-1e-8), "norm_eps")):
        _refused(lambda: normuon_hparams(**kw), word)
    empty, hp = MuonSet(np.zeros((0, 8), np.uint64), _lib.ZS_BF16), normuon_hparams()
    _refused(lambda: empty.run_normuon(hp, 0), "row state")  # a plain Muon set
    _refused(lambda: empty.rows(0), "row state")
    _refused(lambda: empty.attach_rows([1 << 20]), "addresses")
    empty.attach_rows([])
    assert empty.scratch_bytes == 0
    empty.run_normuon(hp, 0)  # nothing to launch
    _refused(lambda: empty.attach_rows([]), "already")
    _refused(lambda: empty.run_normuon_pass(hp, 6, 0), "pass")
    hp.beta2 = 1.0  # a struct filled by hand gets the same rules
    _refused(lambda: empty.run_normuon(hp, 0), "beta2")


def test_the_class_validates_and_sharded_optimizer_names_it():
    from zero_amd._sharded import optimizer_kind
    from zero_amd.optim import NorMuon

    w = torch.nn.Parameter(torch.zeros(4, 8))
    assert optimizer_kind(NorMuon([w])) == "normuon"
    with pytest.raises(TypeError, match="NorMuon"):
        optimizer_kind(torch.optim.Adagrad([w]))
    for kw in (dict(lr=-1.0), dict(beta2=1.0), dict(norm_eps=-1.0), dict(momentum=-0.5)):
        with pytest.raises(ValueError):
            NorMuon([w], **kw)
    with pytest.raises(ValueError, match="2D"):
        NorMuon([torch.nn.Parameter(torch.zeros(8))])
