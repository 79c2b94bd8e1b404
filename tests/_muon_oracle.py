"""torch.optim.Muon's update restated in float64 (torch/optim/_muon.py: _single_tensor_muon,
_zeropower_via_newtonschulz, _adjust_lr).  ``exact``: the normalised bf16 X, then the iteration
without rounding; ``rounded``: bf16 rounding at torch's three points per iteration (the outputs of
``@`` and the two ``addmm``), products accumulated in float64."""
import math

import numpy as np
import torch

COEFFS = (3.4445, -4.7750, 2.0315)


def bf16(x):
    """Round to bf16 (through fp32, to nearest even); float64 out."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().double().numpy()


def lerp(a, b, w):
    """ATen's lerp in float64."""
    return a + w * (b - a) if abs(w) < 0.5 else b - (b - a) * (1 - w)


def normalised(u, eps=1e-7):
    """bf16(u), transposed if tall, divided in fp32 by bf16(max(norm, eps)), rounded to bf16."""
    x = bf16(u)
    if x.shape[0] > x.shape[1]:
        x = x.T
    n = bf16(np.array([max(math.sqrt(float((x * x).sum())), eps)]))[0]
    return bf16(x.astype(np.float32) / np.float32(n))


def newton_schulz(u, coeffs=COEFFS, steps=5, eps=1e-7, rounded=False):
    """The orthogonalised update in u's orientation."""
    a, b, c = coeffs
    rnd = bf16 if rounded else (lambda v: v)
    x = normalised(u, eps)
    for _ in range(steps):
        A = rnd(x @ x.T)
        B = rnd(b * A + c * (A @ A))
        x = rnd(a * x + B @ x)
    return x.T if u.shape[0] > u.shape[1] else x


def adjusted_lr(lr, fn, shape):
    A, B = shape
    return lr * (math.sqrt(max(1, A / B)) if fn in (None, "original") else 0.2 * math.sqrt(max(A, B)))


def step(p, g, buf, *, lr, weight_decay, momentum, nesterov, adjust_lr_fn=None, coeffs=COEFFS,
         steps=5, eps=1e-7):
    """One float64 step with the exact iteration: (p, buf) after it."""
    buf = lerp(buf, g, 1 - momentum)
    u = lerp(g, buf, momentum) if nesterov else buf
    o = newton_schulz(u, coeffs, steps, eps)
    return p * (1 - lr * weight_decay) - adjusted_lr(lr, adjust_lr_fn, p.shape) * o, buf
