"""The C ABI of the per-parameter gradient norms without a GPU: the symbols, their argument checks
(nothing is launched for any of them), the slot rule of an empty set and the numpy restatement of
zs_param_norms against the norm line of zs_clip_coef's restatement."""
import ctypes
import re

import numpy as np

from conftest import REPO
from test_gpu_gradnorm import _coef_ref

NEW = ("zs_adamset_sqnorm_seg_partials", "zs_adamset_grad_sqnorm_segs", "zs_sqnorm_reduce_params",
       "zs_param_norms")


def param_norms_ref(sumsq_vec, div):
    """include/zero_amd.h zs_param_norms, restated."""
    with np.errstate(all="ignore"):
        return (np.sqrt(np.asarray(sumsq_vec, np.float32).astype(np.float64))
                / np.float64(div)).astype(np.float32)


def test_symbols_are_exported_and_declared():
    from zero_amd import _lib

    text = (REPO / "include" / "zero_amd.h").read_text()
    raw = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in NEW:
        assert re.search(rf"^int {name}\(", text, re.M), name
        assert name in _lib.EXPORTED and name in _lib._SIGS, name
        assert hasattr(raw, name), name
    assert _lib.lib.zs_abi_version() == _lib.ABI_VERSION == 13  # additive
    blob = _lib.LIB_PATH.read_bytes()
    for kernel in (b"grad_sqnorm_segs_kernel", b"grad_sqnorm_segs_scalar_kernel",
                   b"sqnorm_reduce_params_kernel", b"param_norms_kernel"):
        assert kernel in blob, kernel


def test_argument_checks_launch_nothing():
    from zero_amd import _lib
    from zero_amd._lib import AdamSeg

    L, INV = _lib.lib, _lib.ZS_ERR_INVALID
    h = ctypes.c_void_p()
    _lib.call("zs_adamset_create", (AdamSeg * 1)(), 0, _lib.ZS_F32, _lib.ZS_BF16, ctypes.byref(h))
    try:
        n = ctypes.c_int64(-1)
        off = (ctypes.c_int64 * 1)(-1)
        _lib.call("zs_adamset_sqnorm_seg_partials", h, ctypes.byref(n), off)
        assert n.value == 0 and off[0] == 0  # an empty set: no slots
        _lib.call("zs_adamset_grad_sqnorm_segs", h, None, 0)  # nothing to write or launch
        fake = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its checks
        for name, args, text in (
                ("zs_adamset_sqnorm_seg_partials", (None, ctypes.byref(n), off), b"NULL"),
                ("zs_adamset_sqnorm_seg_partials", (h, None, off), b"NULL"),
                ("zs_adamset_sqnorm_seg_partials", (h, ctypes.byref(n), None), b"NULL"),
                ("zs_adamset_grad_sqnorm_segs", (None, fake, 0), b"NULL"),
                ("zs_sqnorm_reduce_params", (fake, None, fake, fake, 3, fake, 0), b"NULL"),
                ("zs_sqnorm_reduce_params", (fake, fake, fake, fake, 3, None, 0), b"NULL"),
                ("zs_sqnorm_reduce_params", (fake, fake, fake, fake, -1, fake, 0), b"-1 parameters"),
                ("zs_param_norms", (None, 3, 1.0, fake, 0), b"NULL"),
                ("zs_param_norms", (fake, 3, 1.0, None, 0), b"NULL"),
                ("zs_param_norms", (fake, -1, 1.0, fake, 0), b"-1 elements"),
                ("zs_param_norms", (fake, 3, 0.0, fake, 0), b"grad_div"),
                ("zs_param_norms", (fake, 3, -2.0, fake, 0), b"grad_div")):
            assert getattr(L, name)(*args) == INV, (name, args)
            msg = L.zs_last_error()
            assert msg.startswith(name.encode()) and text in msg, msg
        # nothing to do is not an error, and launches nothing
        assert L.zs_sqnorm_reduce_params(None, fake, None, None, 0, fake, 0) == _lib.ZS_OK
        assert L.zs_param_norms(None, 0, 2.0, None, 0) == _lib.ZS_OK
    finally:
        _lib.call("zs_adamset_destroy", h)


def test_param_norms_restatement_is_the_coefficient_kernels_norm_line():
    """Per element, zs_param_norms is out2[0] of zs_clip_coef: the same double square root and
    division, rounded once — also for 0, inf, NaN and a divisor that is no power of two."""
    rng = np.random.default_rng(3)
    sumsq = np.concatenate([rng.random(64).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 64),
                            np.array([0.0, np.inf, np.nan, 1e-45, 3.4e38], np.float32)])
    for div in (1.0, 2.0, 3.0, 8.0):
        got = param_norms_ref(sumsq, div)
        want = np.array([_coef_ref(s, div, 1.0)[0] for s in sumsq], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), div
    assert param_norms_ref([0.0], 2.0).view(np.uint32)[0] == 0  # +0.0
