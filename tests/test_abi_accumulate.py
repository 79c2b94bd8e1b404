"""zs_accumulate's C ABI without a GPU: the symbol, its argument checks (nothing is launched for
any of them) and the ``accumulate_nt`` knob."""
import ctypes
import re

import numpy as np
import pytest

from conftest import REPO


def test_symbol_is_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    assert re.search(r"^int zs_accumulate\(void\* dst, const void\* src, int64_t n, int dtype, "
                     r"uintptr_t stream\);", text, re.M)
    assert "zs_accumulate" in _lib.EXPORTED and "zs_accumulate" in _lib._SIGS
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "zs_accumulate")
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    assert b"accumulate_kernel" in _lib.LIB_PATH.read_bytes()


def test_argument_checks_launch_nothing():
    from zero_amd import _lib

    lib = _lib.lib
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    p += -p % 16  # a 16-byte aligned host address: every call below returns before a launch
    assert lib.zs_accumulate(p, p + 64, 0, _lib.ZS_F32, 0) == _lib.ZS_OK
    assert lib.zs_accumulate(None, None, 0, _lib.ZS_BF16, 0) == _lib.ZS_OK
    for args, text in (((p, p + 64, 4, _lib.ZS_U8, 0), b"bad dtype"),
                       ((p, p + 64, 4, _lib.ZS_BF16_SPLIT, 0), b"bad dtype"),
                       ((p, p + 64, 4, 7, 0), b"bad dtype"),
                       ((p, p + 64, -1, _lib.ZS_F32, 0), b"n < 0"),
                       ((None, p, 4, _lib.ZS_F32, 0), b"NULL"),
                       ((p, None, 4, _lib.ZS_BF16, 0), b"NULL"),
                       ((p + 4, p + 64, 4, _lib.ZS_F32, 0), b"16-byte aligned"),
                       ((p, p + 66, 4, _lib.ZS_BF16, 0), b"16-byte aligned")):
        assert lib.zs_accumulate(*args) == _lib.ZS_ERR_INVALID, args
        msg = lib.zs_last_error()
        assert msg.startswith(b"zs_accumulate") and text in msg, msg


def test_knob_validates_and_restores():
    from zero_amd import _lib

    lib = _lib.lib
    prev = ctypes.c_int64(99)
    for good in (0, 1):
        assert lib.zs_tune(b"accumulate_nt", good, ctypes.byref(prev)) == _lib.ZS_OK
        assert prev.value == -1
        for bad in (2, -2):
            assert lib.zs_tune(b"accumulate_nt", bad, None) == _lib.ZS_ERR_INVALID
            assert b"out of range" in lib.zs_last_error()
        assert lib.zs_tune(b"accumulate_nt", -1, ctypes.byref(prev)) == _lib.ZS_OK
        assert prev.value == good


def test_wrapper_checks_before_the_library():
    """kernels.accumulate refuses mismatched tensors in Python (CPU tensors: nothing is launched)."""
    import torch

    from zero_amd.kernels import accumulate

    a = torch.zeros(8)
    with pytest.raises(ValueError):
        accumulate(a, torch.zeros(7))
    with pytest.raises(ValueError):
        accumulate(a, torch.zeros(8, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        accumulate(torch.zeros(4, 4).t(), torch.zeros(4, 4))
