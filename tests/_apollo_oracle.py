"""zero_amd.optim.Apollo's rule restated: float64 numpy for the reference, and the element-wise fp32
steps (lerp, the V fma) restated exactly for bit comparisons.  The sign matrix comes from a numpy
lowbias32 of this file's own."""
import numpy as np

U32 = np.uint32


def lowbias32(x):
    x = x ^ (x >> U32(16))
    x = x * U32(0x7feb352d)
    x = x ^ (x >> U32(15))
    x = x * U32(0x846ca68b)
    return x ^ (x >> U32(16))


def keys(seed, epoch):
    w = lambda v: np.array([v & 0xFFFFFFFF], U32)  # noqa: E731
    k0 = lowbias32(w(epoch) ^ w(seed))
    return k0, lowbias32((k0 ^ w(seed >> 32) ^ w(epoch >> 32)) + U32(0x9E3779B9))


def sigma(K, rank, seed, epoch):
    """K x rank, float64 +-1: +1 where bit (k & 31) of bits((j << 32) | (k >> 5)) is 0."""
    k0, k1 = keys(seed, epoch)
    k, j = np.arange(K, dtype=U32)[:, None], np.arange(rank, dtype=U32)[None, :]
    h = lowbias32((k >> U32(5)) ^ k0 ^ (j * U32(0x9E3779B9))) ^ k1
    return 1.0 - 2.0 * ((h >> (k & U32(31))) & U32(1)).astype(np.float64)


def channels(x):
    """An R x C array as N x K: rows are channels when R >= C, columns otherwise."""
    return x if x.shape[0] >= x.shape[1] else x.T


def fma32(a, b, c):
    """fp32 fma(a, b, c), correctly rounded: the exact product and a TwoSum in float64, the sum
    rounded to odd before the one rounding to fp32."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def moments32(M, V, S, beta1, beta2):
    """The kernel's M and V after S, in fp32: ATen's two-range lerp as one fma, V as one fma."""
    w = np.float32(1.0 - beta1)
    M = fma32(w, S - M, M) if abs(w) < 0.5 else fma32(w - np.float32(1), S - M, S)
    return M, fma32(np.float32(1.0 - beta2), S * S, V * np.float32(beta2))


def scalars(M, V, S, gg, Fp, t, *, lr, beta1, beta2, eps, scale=1.0, scale_type="channel",
            norm_growth=1.01, **_):
    """(a_c, F_prev after, lam) in float64 from the moments, the sketch and the channels' sums of
    g^2."""
    Nh = (M / (1 - beta1 ** t)) / (np.sqrt(V) / np.sqrt(1 - beta2 ** t) + eps)
    nn, ss = (Nh ** 2).sum(1), (S ** 2).sum(1)
    if scale_type == "tensor":
        nn, ss = np.full_like(nn, nn.sum()), np.full_like(ss, ss.sum())
    s = np.sqrt(nn) / (np.sqrt(ss) + 1e-8)
    F = np.sqrt((s * s * gg).sum())
    lam = max(F / (Fp + 1e-8), norm_growth) / norm_growth if norm_growth > 0 and Fp > 0 else 1.0
    return -lr * np.sqrt(scale) * s / lam, F / lam, lam


def step(p, g, M, V, Fp, t, *, seed, rank, update_proj_gap, weight_decay=0.0, **hp):
    """One float64 step on the gradient ``g`` (R x C) at step count ``t`` (after the step):
    (p, M, V, F_prev) after it."""
    import torch

    G = channels(g)
    Gb = channels(torch.from_numpy(g.astype(np.float32)).to(torch.bfloat16).double().numpy())
    S = (Gb @ sigma(G.shape[1], rank, seed, (t - 1) // update_proj_gap)) / np.sqrt(rank)
    M = M + (1 - hp["beta1"]) * (S - M)
    V = hp["beta2"] * V + (1 - hp["beta2"]) * S * S
    a, Fp, _ = scalars(M, V, S, (G ** 2).sum(1), Fp, t, **hp)
    upd = a[:, None] * G
    return p * (1 - hp["lr"] * weight_decay) + (upd if g.shape[0] >= g.shape[1] else upd.T), M, V, Fp
