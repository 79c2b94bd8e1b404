"""The fused LAMB's C entry points on the host: the symbols resolve, NULL and bad arguments return
ZS_ERR_INVALID (nothing is launched before the checks), the ABI version stays 13."""
import ctypes

import pytest

from zero_amd import _lib
from zero_amd._lib import LambHParams

GOOD = (0.9, 0.999, 1e-6, 0.01, 1, 0, 2, 3.0)  # beta1, beta2, eps, wd, bias_correction, maximize, t, div


def test_symbols_version_and_hparams():
    assert _lib.lib.zs_abi_version() == 13
    hp = LambHParams()
    _lib.call("zs_lamb_hparams_init", *GOOD, ctypes.byref(hp))
    assert hp.bc1 == pytest.approx(1 - 0.9 ** 2) and hp.bc2_sqrt == pytest.approx((1 - 0.999 ** 2) ** 0.5)
    assert hp.grad_div == 3.0 and hp.maximize == 0
    _lib.call("zs_lamb_hparams_init", 0.9, 0.999, 1e-6, 0.0, 0, 1, 5, 1.0, ctypes.byref(hp))
    assert hp.bc1 == 1.0 and hp.bc2_sqrt == 1.0 and hp.maximize == 1


@pytest.mark.parametrize("name,args", [
    ("zs_lamb_hparams_init", GOOD + (None,)),
    *[("zs_lamb_hparams_init", GOOD[:j] + (bad,) + GOOD[j + 1:] + (ctypes.byref(LambHParams()),))
      for j, bad in ((0, 1.0), (1, -0.1), (2, -1.0), (3, -1.0), (6, 0), (7, 0.0))],
    ("zs_lambset_run_moments", (None, ctypes.byref(LambHParams()), None, None, 0)),
    ("zs_lambset_run_apply", (None, ctypes.byref(LambHParams()), None, 0, 0)),
    ("zs_lambset_bind_params", (None, 0, None)),
    ("zs_lamb_finish", (None, 4, None, None, None, None, 0)),
    ("zs_lamb_finish", (None, -1, None, None, None, None, 0))])
def test_bad_arguments(name, args):
    with pytest.raises(_lib.ZeroAmdError) as e:
        _lib.call(name, *args)
    assert e.value.code == _lib.ZS_ERR_INVALID
