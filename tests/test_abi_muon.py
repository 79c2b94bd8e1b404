"""The fused Muon's C ABI without a GPU: the symbols, and the argument checks that come before any
allocation, upload or launch."""
import ctypes
import re

import numpy as np
import pytest

from conftest import REPO

NAMES = ("zs_muon_hparams_init", "zs_muonset_create", "zs_muonset_run", "zs_muonset_run_pass",
         "zs_muonset_stats", "zs_muonset_batch", "zs_muonset_destroy", "zs_muon_gemm_nt")


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    integration = (REPO / "INTEGRATION.md").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert name in _lib.EXPORTED and name in _lib._SIGS and hasattr(so, name)
        assert re.search(rf"^int {name}\(", text, re.M) and name in integration
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    assert b"muon_gemm_nt_kernel" in _lib.LIB_PATH.read_bytes()  # the kernels are in the code object
    assert ctypes.sizeof(_lib.MuonSeg) == 64 and ctypes.sizeof(_lib.MuonHParams) == 80


def _refused(fn, word):
    from zero_amd import _lib

    with pytest.raises(_lib.ZeroAmdError) as e:
        fn()
    assert e.value.code == _lib.ZS_ERR_INVALID and word in str(e.value), str(e.value)


def test_hparams_create_run_and_product_refuse_without_a_device():
    """Host addresses stand in for device ones: every call returns before an allocation or launch."""
    from zero_amd import _lib
    from zero_amd.kernels import MuonSet, muon_hparams

    a = 1 << 20
    for kw, word in ((dict(ns_steps=100), "Newton-Schulz"), (dict(ns_steps=-1), "Newton-Schulz"),
                     (dict(lr=-1.0), "learning rate"), (dict(momentum=-0.1), "momentum"),
                     (dict(weight_decay=-0.1), "weight decay"), (dict(grad_div=0.0), "grad_div")):
        _refused(lambda: muon_hparams(**kw), word)

    def row(**k):
        r = dict(g=a, master=a, master_out=a, p_out=0, buf=a, R=4, C=8, param=0)
        r.update(k)
        return [r[f] for f in MuonSet.FIELDS]

    make = lambda rows, g=_lib.ZS_BF16, p=_lib.ZS_BF16, **kw: MuonSet(np.array(rows, np.uint64), g, p, **kw)  # noqa: E731
    for args, kw, word in ((([], 7), {}, "g_dtype"), (([], _lib.ZS_BF16, _lib.ZS_BF16_SR), {}, "p_dtype"),
                           (([row(g=0)],), {}, "missing"), (([row(buf=0)],), {}, "missing"),
                           (([row(R=0)],), {}, "R and C"), (([row(master_out=a + 64)],), {}, "in place"),
                           (([row()], _lib.ZS_BF16, _lib.ZS_BF16_SPLIT), {}, "split master needs p_out"),
                           (([row(g=a + 1)],), {}, "aligned"), (([row(buf=a + 2)],), {}, "aligned"),
                           (([row(R=512, C=512)],), dict(scratch_budget=1 << 20), "budget")):
        _refused(lambda: make(*args, **kw), word)
    empty, hp = make([]), muon_hparams()
    assert (empty.elems, empty.batches, empty.scratch_bytes) == (0, 0, 0)
    empty.run(hp, 0)  # nothing to launch
    hp.ns_steps = 100  # a struct filled by hand gets the same rules
    _refused(lambda: empty.run(hp, 0), "Newton-Schulz")
    _refused(lambda: _lib.call("zs_muonset_run", None, ctypes.byref(muon_hparams()), 0), "NULL")
    _refused(lambda: empty.run_pass(muon_hparams(), 4, 0), "pass")
    base = dict(A=a, lda=8, B=a + 4096, ldb=8, E=0, lde=0, D=a + 8192, ldd=8, D2=0, ldd2=0, M=8, N=8, K=8,
                alpha=1.0, beta=0.0, sym=0, stream=0)
    gemm = lambda **k: _lib.call("zs_muon_gemm_nt", *{**base, **k}.values())  # noqa: E731
    for kw, word in ((dict(A=0), "NULL"), (dict(D=a + 8193), "aligned"), (dict(lda=4), "row stride"),
                     (dict(beta=1.0), "needs E"), (dict(sym=1, N=4), "symmetric"), (dict(D=a), "aliases")):
        _refused(lambda: gemm(**kw), word)
