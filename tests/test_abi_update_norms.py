"""The C ABI of the per-parameter update and weight norms without a GPU: the three symbols, their
argument checks (nothing is launched for any of them) and the slot rule of an empty set.  (The
refusals that need a set with segments -- the carry, the vmax column, NULL partials for a set with
slots -- are in tests/test_gpu_update_norms_kernel.py: a table with segments is uploaded to the
device.)"""
import ctypes
import re

import numpy as np

from conftest import REPO

NEW = ("zs_adamset_update_norm_slots", "zs_adamset_run_stats", "zs_update_norms")


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert re.search(rf"^int {name}\(", text, re.M), name
        assert name in _lib.EXPORTED and name in _lib._SIGS, name
        assert hasattr(raw, name), name
        assert name in (REPO / "INTEGRATION.md").read_text(), name
    assert re.search(r"^int zs_adamset_run_stats\(const zs_adamset\* as, const zs_adam_hparams\* hp, "
                     r"const float\* coef,\s+int guard, double\* partials, uintptr_t stream\);",
                     text, re.M)
    assert re.search(r"^#define ZS_ABI_VERSION 13$", text, re.M)
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    blob = _lib.LIB_PATH.read_bytes()
    for kernel in (b"AdamStatsRule", b"update_norms_kernel"):  # the instances are in the code object
        assert kernel in blob, kernel


def _empty_set(create, *args):
    from zero_amd import _lib

    h = ctypes.c_void_p()
    _lib.call(create, None, 0, *args, ctypes.byref(h))  # no segments: nothing is uploaded
    return h


def test_argument_checks_launch_nothing():
    from zero_amd import _lib

    lib, INV = _lib.lib, _lib.ZS_ERR_INVALID
    buf = np.zeros(16, np.float64)
    p = buf.ctypes.data  # a host address: every call below returns before a launch
    hp, ams = _lib.AdamHParams(), _lib.AdamHParams()
    ams.amsgrad = 1
    plain = _empty_set("zs_adamset_create", _lib.ZS_BF16, _lib.ZS_BF16_SPLIT)
    sgd = _empty_set("zs_sgdset_create", _lib.ZS_BF16, _lib.ZS_BF16_SPLIT)
    bf16_state = _empty_set("zs_adamset_create_ex", _lib.ZS_BF16, _lib.ZS_BF16_SPLIT, _lib.ZS_BF16)
    psr = _empty_set("zs_adamset_create_ex", _lib.ZS_BF16, _lib.ZS_BF16_SR, _lib.ZS_F32)
    n = ctypes.c_int64(-1)
    off = (ctypes.c_int64 * 1)(-1)
    ref = ctypes.byref
    try:
        _lib.call("zs_adamset_update_norm_slots", plain, ref(n), off)
        assert n.value == 0 and off[0] == 0  # an empty set: no slots
        cases = (
            ("zs_adamset_update_norm_slots", (None, ref(n), off), b"NULL"),
            ("zs_adamset_update_norm_slots", (plain, None, off), b"NULL"),
            ("zs_adamset_update_norm_slots", (plain, ref(n), None), b"NULL"),
            ("zs_adamset_run_stats", (None, ref(hp), p, 0, p, 0), b"NULL"),
            ("zs_adamset_run_stats", (plain, None, p, 0, p, 0), b"NULL"),
            ("zs_adamset_run_stats", (sgd, ref(hp), p, 0, p, 0), b"zs_sgdset_create"),
            ("zs_adamset_run_stats", (bf16_state, ref(hp), p, 0, p, 0), b"ZS_BF16 state"),
            ("zs_adamset_run_stats", (psr, ref(hp), p, 0, p, 0), b"ZS_BF16_SR"),
            ("zs_adamset_run_stats", (plain, ref(ams), p, 0, p, 0), b"amsgrad"),
            ("zs_adamset_run_stats", (plain, ref(hp), None, 1, p, 0), b"guard"),
            ("zs_update_norms", (None, 3, None, p, p, 0), b"NULL"),
            ("zs_update_norms", (p, 3, None, None, p, 0), b"NULL"),
            ("zs_update_norms", (p, 3, None, p, None, 0), b"NULL"),
            ("zs_update_norms", (p, -1, None, p, p, 0), b"-1 parameters"),
        )
        for name, args, text in cases:
            assert getattr(lib, name)(*args) == INV, (name, args)
            msg = lib.zs_last_error()
            assert msg.startswith(name.encode() + b":") and text in msg, msg
        # an empty set has nothing to launch, with or without a coefficient or partials
        assert lib.zs_adamset_run_stats(plain, ref(hp), None, 0, None, 0) == _lib.ZS_OK
        assert lib.zs_adamset_run_stats(plain, ref(hp), p, 1, None, 0) == _lib.ZS_OK
        assert lib.zs_update_norms(None, 0, None, None, None, 0) == _lib.ZS_OK
    finally:
        for h in (plain, sgd, bf16_state, psr):
            lib.zs_adamset_destroy(h)
    assert not buf.any()
