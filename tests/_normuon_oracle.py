"""zero_amd.optim.NorMuon's update restated in float64, on tests/_muon_oracle.py's unrounded
Newton-Schulz iteration."""
import numpy as np

import _muon_oracle as mo


def step(p, g, buf, v, *, lr, weight_decay, momentum, nesterov, beta2=0.95, norm_eps=1e-8):
    """One float64 step: (p, buf, v) after it."""
    buf = mo.lerp(buf, g, 1 - momentum)
    o = mo.newton_schulz(mo.lerp(g, buf, momentum) if nesterov else buf)
    v = mo.lerp(v, (o * o).mean(axis=1), 1 - beta2)
    on = o / (np.sqrt(v) + norm_eps)[:, None]
    f = np.linalg.norm(on)
    s = 0.0 if f == 0 else 0.2 * lr * np.sqrt(p.size) / f
    return p * (1 - lr * weight_decay) - s * on, buf, v
