"""zero_amd.optim.AdamMini's update restated in float64: the reference of the fused Adam-mini
kernels."""
import numpy as np


def blocks(shape, block_rows):
    return 1 if len(shape) < 2 or block_rows == 0 else shape[0] // block_rows


def step(p, g, m, v, t, nblk, *, lr, beta1, beta2, eps, weight_decay):
    """One float64 step on the averaged gradient ``g`` at step count ``t`` (after the step), the
    parameter cut into ``nblk`` blocks: (p, m, v, a) after it, a the step of every block."""
    m = m + (1 - beta1) * (g - m)
    v = v * beta2 + (1 - beta2) * (g.reshape(nblk, -1) ** 2).mean(axis=1)
    a = -(lr / (1 - beta1 ** t)) / (np.sqrt(v) / np.sqrt(1 - beta2 ** t) + eps)
    p = p * (1 - lr * weight_decay) + (a[:, None] * m.reshape(nblk, -1)).reshape(p.shape)
    return p, m, v, a
