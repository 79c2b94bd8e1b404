"""tests/_adafactor_oracle.py against torch.optim.Adafactor(foreach=False) on float64 parameters
(eps1 passed explicitly: torch would otherwise take float64's epsilon), within 1e-12 relative."""
import zlib

import numpy as np
import pytest
import torch

import _adafactor_oracle as ao

SHAPES = [(37, 53), (70, 520), (1, 300), (300, 1), (4100, 8), (3, 4104), (2, 33, 40), (1000,), (63,)]
CASES = {
    "plain": dict(),
    "maximize_decay": dict(maximize=True, weight_decay=0.1),
    "zero_grad": dict(),
    "zero_param": dict(),
}


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_oracle_is_torch_float64(shape, case, t):
    rng = np.random.default_rng(zlib.crc32(repr((shape, case, t)).encode()))
    kw = dict(lr=1e-2, beta2_decay=-0.8, eps2=1e-3, d=1.0, weight_decay=0.0, maximize=False)
    kw.update(CASES[case])
    p0 = np.zeros(shape) if case == "zero_param" else rng.standard_normal(shape) * 0.05
    g = np.zeros(shape) if case == "zero_grad" else rng.standard_normal(shape) * 1e-2
    state = ao.zero_state(shape) if t == 1 else \
        {k: rng.random(v.shape) * 1e-4 for k, v in ao.zero_state(shape).items()}
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adafactor([p], lr=kw["lr"], beta2_decay=kw["beta2_decay"],
                                eps=(ao.EPS1_F32, kw["eps2"]), d=kw["d"],
                                weight_decay=kw["weight_decay"], maximize=kw["maximize"],
                                foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)),
                    **{k: torch.from_numpy(v.copy()) for k, v in state.items()}}
    p.grad = torch.from_numpy(g.copy())
    opt.step()
    want_p, want_state, _ = ao.step(p0, g, state, t, eps1=ao.EPS1_F32, **kw)
    pairs = [(p.detach().numpy(), want_p)] + [(opt.state[p][k].numpy(), v) for k, v in want_state.items()]
    for got, want in pairs:
        assert np.max(np.abs(got - want)) <= 1e-12 * max(np.max(np.abs(want)), 1e-300)
