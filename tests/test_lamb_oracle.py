"""zero_amd.optim.LAMB.step() on fp32 CPU tensors against its numpy restatement (tests/_lamb_oracle.py):
m and v bit for bit over three steps, and p bit for bit when the oracle applies the -s that step()
applied (the two compute the norms in different orders: the ratio itself agrees to fp32 rounding)."""
import numpy as np
import pytest
import torch

import _lamb_oracle as lo
from zero_amd.optim import LAMB


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_step_equals_oracle(wd, bias_correction, maximize):
    rng = np.random.default_rng(5)
    n, lr, betas, eps = 4099, 2e-3, (0.9, 0.999), 1e-6
    p0 = rng.standard_normal(n).astype(np.float32)
    p = torch.from_numpy(p0.copy()).requires_grad_()
    opt = LAMB([p], lr=lr, betas=betas, eps=eps, weight_decay=wd, bias_correction=bias_correction,
               maximize=maximize)
    po, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in (1, 2, 3):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, n)).astype(np.float32)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        hp = lo.LambHP(lr, *betas, eps, wd, t, bias_correction=bias_correction, maximize=maximize)
        r = float(opt.last_trust_ratios[p])
        neg_s = -(np.float32(lr) * np.float32(r))
        po, m, v, _, (_, _, r_o, _) = lo.step(po, g, m, v, hp, neg_s=neg_s)
        st = opt.state[p]
        assert np.array_equal(st["exp_avg"].numpy().view(np.uint32), m.view(np.uint32))
        assert np.array_equal(st["exp_avg_sq"].numpy().view(np.uint32), v.view(np.uint32))
        assert np.array_equal(p.detach().numpy().view(np.uint32), po.view(np.uint32))
        assert abs(r - float(r_o)) <= 8 * 2.0 ** -24 * r  # two summation orders of n fp32 squares
        assert float(st["step"]) == t

