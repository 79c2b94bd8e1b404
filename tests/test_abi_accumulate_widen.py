"""zs_accumulate_widen's C ABI without a GPU: the symbol, its argument checks (nothing is launched
for any of them), the shared ``accumulate_nt`` knob, and the Python wrapper's own refusals."""
import ctypes
import re

import numpy as np
import pytest

from conftest import REPO


def test_symbol_is_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    assert re.search(r"^int zs_accumulate_widen\(float\* dst, const void\* a_bf16, "
                     r"const void\* src_bf16, int64_t n,\s+uintptr_t stream\);", text, re.M)
    assert "zs_accumulate_widen" in (REPO / "INTEGRATION.md").read_text()
    assert "zs_accumulate_widen" in _lib.EXPORTED and "zs_accumulate_widen" in _lib._SIGS
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "zs_accumulate_widen")
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    assert b"accumulate_widen_kernel" in _lib.LIB_PATH.read_bytes()


def test_argument_checks_launch_nothing():
    from zero_amd import _lib

    lib = _lib.lib
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    p += -p % 16  # a 16-byte aligned host address: every call below returns before a launch
    a, s = p + 64, p + 128
    assert lib.zs_accumulate_widen(p, a, s, 0, 0) == _lib.ZS_OK
    assert lib.zs_accumulate_widen(p, None, s, 0, 0) == _lib.ZS_OK
    assert lib.zs_accumulate_widen(None, None, None, 0, 0) == _lib.ZS_OK
    for args, text in (((p, a, s, -1, 0), b"n < 0"),
                       ((p, None, s, -5, 0), b"n < 0"),
                       ((None, a, s, 4, 0), b"NULL"),
                       ((p, a, None, 4, 0), b"NULL"),
                       ((None, None, s, 4, 0), b"NULL"),
                       ((p + 4, a, s, 4, 0), b"16-byte aligned"),
                       ((p + 8, None, s, 4, 0), b"16-byte aligned"),
                       ((p, a + 2, s, 4, 0), b"8-byte aligned"),
                       ((p, a + 4, s, 4, 0), b"8-byte aligned"),
                       ((p, a, s + 2, 4, 0), b"8-byte aligned"),
                       ((p, None, s + 4, 4, 0), b"8-byte aligned")):
        assert lib.zs_accumulate_widen(*args) == _lib.ZS_ERR_INVALID, args
        msg = lib.zs_last_error()
        assert msg.startswith(b"zs_accumulate_widen") and text in msg, msg


def test_knob_is_the_accumulate_one():
    """No knob of its own: ``accumulate_nt`` covers both kernels, and nothing else was added."""
    from zero_amd import _lib

    lib = _lib.lib
    prev = ctypes.c_int64(99)
    assert lib.zs_tune(b"accumulate_nt", 1, ctypes.byref(prev)) == _lib.ZS_OK and prev.value == -1
    assert lib.zs_tune(b"accumulate_nt", -1, ctypes.byref(prev)) == _lib.ZS_OK and prev.value == 1
    assert lib.zs_tune(b"accumulate_widen_nt", 1, None) == _lib.ZS_ERR_INVALID


def test_set_wrappers_take_fp32_grads_over_the_split_master_only_by_name():
    """AdamSet / SgdSet keep refusing ZS_F32 gradients over ZS_BF16_SPLIT, as before the library
    accepted them, unless ``wide_grads=True``; the refusal is the wrapper's (nothing reaches the
    library, so no device is needed)."""
    from zero_amd import _lib
    from zero_amd.kernels import AdamSet, SgdSet

    _lib.lib.zs_accumulate_widen(None, None, None, -1, 0)  # leaves "n < 0" as the last error
    before = _lib.lib.zs_last_error()
    row = np.array([[4096, 8192, 12288, 8192, 16384, 20480, 0, 0, 64]], np.uint64)  # never read
    for mk in (AdamSet, SgdSet):
        with pytest.raises(_lib.ZeroAmdError, match="bf16 grads") as e:
            mk(row, _lib.ZS_F32, _lib.ZS_BF16_SPLIT)
        assert e.value.code == _lib.ZS_ERR_INVALID and mk._CREATE in str(e.value)
        with pytest.raises(_lib.ZeroAmdError, match="bf16 grads"):
            mk(row, _lib.ZS_F32, _lib.ZS_BF16_SPLIT, wide_grads=False)
    assert _lib.lib.zs_last_error() == before


def test_wrapper_checks_before_the_library():
    """kernels.accumulate_widen refuses mismatched tensors in Python (CPU tensors: nothing is
    launched, and the library's own message never appears)."""
    import torch

    from zero_amd import _lib
    from zero_amd.kernels import accumulate_widen

    _lib.lib.zs_accumulate_widen(None, None, None, -1, 0)  # leaves "n < 0" as the last error
    before = _lib.lib.zs_last_error()
    d, s = torch.zeros(8), torch.zeros(8, dtype=torch.bfloat16)
    for args in ((d, torch.zeros(7, dtype=torch.bfloat16)),            # count
                 (d, s, torch.zeros(9, dtype=torch.bfloat16)),         # count of a
                 (d, torch.zeros(8)),                                  # src not bf16
                 (s, s),                                               # dst not fp32
                 (d, s, torch.zeros(8)),                               # a not bf16
                 (torch.zeros(4, 4).t(), torch.zeros(16, dtype=torch.bfloat16)),   # not contiguous
                 (torch.zeros(12)[1:9], s),                            # dst 4 bytes off
                 (d, torch.zeros(12, dtype=torch.bfloat16)[1:9]),      # src 2 bytes off
                 (d, s, torch.zeros(12, dtype=torch.bfloat16)[2:10])):  # a 4 bytes off
        with pytest.raises(ValueError):
            accumulate_widen(*args)
    assert _lib.lib.zs_last_error() == before
