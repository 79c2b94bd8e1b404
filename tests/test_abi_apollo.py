"""The fused APOLLO's C ABI and host logic without a GPU: the symbols, the argument checks that come
before any allocation, upload or launch, and the class's own checks (the combinations check_apollo
refuses: tests/test_gpu_apollo_optimizer.py)."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from test_abi_adafactor import _refused

NAMES = ("zs_apollo_hparams_init", "zs_apolloset_create", "zs_apolloset_run", "zs_apolloset_run_pass",
         "zs_apolloset_stats", "zs_apolloset_destroy")


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    integration = (REPO / "INTEGRATION.md").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NAMES:
        assert name in _lib.EXPORTED and name in _lib._SIGS and hasattr(so, name)
        assert re.search(rf"^int {name}\(", text, re.M) and name in integration
    assert re.search(r"^#define ZS_ABI_VERSION 13$", text, re.M)
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    code = _lib.LIB_PATH.read_bytes()  # the kernels are in the code object
    assert all(k in code for k in (b"apollo_sketch_kernel", b"apollo_moments_kernel",
                                   b"apollo_finish_kernel", b"apollo_apply_kernel"))
    assert ctypes.sizeof(_lib.ApolloSeg) == 88 and ctypes.sizeof(_lib.ApolloHParams) == 80


@pytest.mark.parametrize("kw,word", [
    (dict(lr=-1.0), "learning rate"), (dict(lr=float("nan")), "learning rate"), (dict(beta1=1.0), "index 0"),
    (dict(beta2=-0.1), "index 1"), (dict(eps=-1e-8), "epsilon"), (dict(weight_decay=-0.1), "weight_decay"),
    (dict(scale=0.0), "scale"), (dict(update_proj_gap=0), "update_proj_gap"),
    (dict(norm_growth=1.0), "norm_growth"), (dict(norm_growth=-2.0), "norm_growth"),
    (dict(grad_div=0.0), "grad_div")])
def test_hparams_init_and_the_class_refuse_the_same(kw, word):
    from zero_amd.kernels import apollo_hparams
    from zero_amd.optim import Apollo

    _refused(lambda: apollo_hparams(**kw), "zs_apollo_hparams_init", word)
    if "grad_div" not in kw:
        ckw = {("betas" if k.startswith("beta") else k): v for k, v in kw.items()}
        if "betas" in ckw:
            ckw["betas"] = (kw.get("beta1", 0.9), kw.get("beta2", 0.999))
        with pytest.raises(ValueError):
            Apollo([torch.nn.Parameter(torch.zeros(8, 4))], **ckw)


def test_the_class_refuses_what_is_not_a_matrix_a_rank_or_a_scale_type():
    from zero_amd.kernels import apollo_hparams
    from zero_amd.optim import Apollo

    p = lambda *s: [torch.nn.Parameter(torch.zeros(*s))]  # noqa: E731
    for shape, kw in (((8,), {}), ((2, 3, 4), {}), ((8, 4), dict(rank=0)), ((8, 4), dict(rank=257)),
                      ((8, 4), dict(rank=1.5)), ((8, 4), dict(scale_type="row"))):
        with pytest.raises(ValueError):
            Apollo(p(*shape), **kw)
    with pytest.raises(ValueError):
        apollo_hparams(scale_type="row")
    h = apollo_hparams()
    assert (h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.scale, h.norm_growth, h.grad_div,
            h.update_proj_gap, h.scale_type, h.maximize) == (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.01, 1.0, 200, 0, 0)
    h.scale_type = 2  # a struct filled by hand gets the same rules
    from zero_amd.kernels import ApolloSet
    _refused(lambda: ApolloSet(np.zeros((0, 11), np.uint64), 1).run(h, 1, 0), "zs_apolloset_run", "scale_type")


def test_create_and_run_refuse_without_a_device():
    """Host addresses stand in for device ones: every call returns before an allocation."""
    from zero_amd import _lib
    from zero_amd.kernels import AdamMiniSet, ApolloSet, adamini_hparams, apollo_hparams

    BF16, SPLIT = _lib.ZS_BF16, _lib.ZS_BF16_SPLIT
    a = 1 << 20

    def row(**k):
        r = dict(g=a, master=a, master_out=a, p_out=0, m=a, v=a, fprev=a, R=4, C=8, seed=0, param=0)
        r.update(k)
        return [r[f] for f in ApolloSet.FIELDS]

    make = lambda rows, g=BF16, p=BF16, **kw: ApolloSet(np.array(rows, np.uint64), g, p, **kw)  # noqa: E731
    for args, kw, word in ((([], 7), {}, "g_dtype"), (([], BF16, _lib.ZS_BF16_SR), {}, "p_dtype"),
                           (([],), dict(rank=0), "rank"), (([],), dict(rank=257), "rank"),
                           (([row(g=0)],), {}, "missing"), (([row(m=0)],), {}, "missing"),
                           (([row(v=0)],), {}, "missing"), (([row(fprev=0)],), {}, "missing"),
                           (([row(R=0)],), {}, "R and C"), (([row(master_out=a + 64)],), {}, "in place"),
                           (([row()], BF16, SPLIT), {}, "split master needs p_out"),
                           (([row(g=a + 1)],), {}, "aligned"), (([row(fprev=a + 2)],), {}, "aligned")):
        _refused(lambda: make(*args, **kw), "zs_apolloset_create", word)
    lib, R = _lib.lib, ctypes.byref
    hp, empty, other = apollo_hparams(), make([]), AdamMiniSet(np.zeros((0, 10), np.uint64), BF16)
    assert (empty.elems, empty.bytes, empty.scratch_bytes, empty.channels) == (0, 0, 0, 0)
    for args, text in (((None, R(hp), 1, 0), b"NULL"), ((empty._h, None, 1, 0), b"NULL"),
                       ((empty._h, R(hp), 0, 0), b"step must be >= 1"),
                       ((other._h, R(hp), 1, 0), b"zs_apolloset_create")):
        assert lib.zs_apolloset_run(*args) == _lib.ZS_ERR_INVALID, args
        msg = lib.zs_last_error()
        assert msg.startswith(b"zs_apolloset_run:") and text in msg, msg
    assert lib.zs_adaminiset_run(empty._h, R(adamini_hparams()), 1, 0) == _lib.ZS_ERR_INVALID
    empty.run(hp, 1, 0)  # an empty set has nothing to launch
    empty.run_pass(hp, 7, 3, 0)
    _refused(lambda: empty.run_pass(hp, 1, 4, 0), "pass")

