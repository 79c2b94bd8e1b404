"""The guarded update's C ABI and the optimizers' argument checks without a GPU: the symbols, their
argument checks (nothing is launched for any of them) and the ValueErrors raised before any device
work."""
import ctypes
import re

import numpy as np
import pytest

from conftest import REPO

NEW = ("zs_clip_coef_guarded", "zs_adamset_run_guarded", "zs_adamset_run_sr_guarded")


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.EXPORTED and name in _lib._SIGS, name
        assert hasattr(so, name), name
    assert re.search(r"^#define ZS_ABI_VERSION 13$", text, re.M)
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    assert b"clip_coef_guarded_kernel" in _lib.LIB_PATH.read_bytes()


def test_argument_checks_launch_nothing():
    from zero_amd import _lib

    lib = _lib.lib
    buf = np.zeros(16, np.float32)
    p = buf.ctypes.data  # a host address: every call below returns before a launch
    hp = _lib.AdamHParams()
    cases = (
        ("zs_clip_coef_guarded", (None, 1.0, 1.0, p, p + 8, 0), b"NULL"),
        ("zs_clip_coef_guarded", (p, 1.0, 1.0, None, p + 8, 0), b"NULL"),
        ("zs_clip_coef_guarded", (p, 1.0, 1.0, p, None, 0), b"NULL"),
        ("zs_clip_coef_guarded", (p, 0.0, 1.0, p, p + 8, 0), b"grad_div"),
        ("zs_clip_coef_guarded", (p, -2.0, 1.0, p, p + 8, 0), b"grad_div"),
        ("zs_clip_coef_guarded", (p, 1.0, -1.0, p, p + 8, 0), b"max_norm"),
        ("zs_clip_coef_guarded", (p, 1.0, float("nan"), p, p + 8, 0), b"max_norm"),
        ("zs_adamset_run_guarded", (None, ctypes.byref(hp), p, 0), b"NULL"),
        ("zs_adamset_run_sr_guarded", (None, ctypes.byref(hp), p, 0, 1, 2, 0), b"NULL"),
    )
    for name, args, text in cases:
        assert getattr(lib, name)(*args) == _lib.ZS_ERR_INVALID, (name, args)
        msg = lib.zs_last_error()
        assert msg.startswith(name.encode() + b":") and text in msg, msg
    assert not buf.any()


def test_check_helpers():
    from zero_amd._update import check_max_grad_norm, check_skip_nonfinite

    for good in (None, 0, 0.0, 1, 2.5, float("inf")):
        check_max_grad_norm(good)
    for bad in (-1.0, float("nan"), "1", True, [1.0]):
        with pytest.raises(ValueError, match="max_grad_norm"):
            check_max_grad_norm(bad)
    assert check_skip_nonfinite(False, None, "sgd") is False
    assert check_skip_nonfinite(True, float("inf"), "adam") is True
    with pytest.raises(ValueError, match="max_grad_norm"):
        check_skip_nonfinite(True, None, "adam")
    with pytest.raises(ValueError, match="SGD"):
        check_skip_nonfinite(True, 1.0, "sgd")


def _adam():
    import torch

    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(8))], lr=1e-3)


def _sgd():
    import torch

    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(8))], lr=1e-3, momentum=0.9)


def test_zero3_constructor_refuses_before_any_device_work():
    """CPU parameters, no process group: each error below comes before the first thing that would
    need either."""
    from zero_amd import zero3

    with pytest.raises(ValueError, match="update mode"):
        zero3.ShardedOptimizer(_adam(), update=False, max_grad_norm=1.0)
    for bad in (-1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="max_grad_norm"):
            zero3.ShardedOptimizer(_adam(), update=True, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        zero3.ShardedOptimizer(_adam(), update=True, skip_nonfinite=True)
    with pytest.raises(ValueError, match="SGD"):
        zero3.ShardedOptimizer(_sgd(), update=True, max_grad_norm=1.0, skip_nonfinite=True)
