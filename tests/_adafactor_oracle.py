"""torch.optim.Adafactor's single-tensor rule (torch/optim/_adafactor.py) restated in numpy, double
throughout: the reference of the fused Adafactor kernels.  tests/test_adafactor_oracle.py pins it
to torch's own float64 run."""
import numpy as np

lerp = lambda a, b, w: a + w * (b - a)  # noqa: E731  (ATen's lerp in exact terms)
EPS1_F32 = 2.0 ** -23


def step(p, g, state, t, *, lr=1e-2, beta2_decay=-0.8, eps1=EPS1_F32, eps2=1e-3, d=1.0,
         weight_decay=0.0, maximize=False):
    """One step on float64 ``p`` with averaged gradient ``g`` at step count ``t`` (after the step).
    ``state``: {"row_var": (..., R, 1), "col_var": (..., 1, C)} or {"variance": (n,)}.  Returns
    (p', state', delta) with delta the update added to the decayed parameter."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    g = -g if maximize else g
    w = float(t) ** beta2_decay
    rho = min(lr, 1.0 / np.sqrt(float(t)))
    alpha = max(eps2, np.sqrt(np.sum(p * p)) / np.sqrt(p.size)) * rho
    if weight_decay != 0:
        p = p * (1.0 - lr * weight_decay)
    if g.ndim > 1:
        row = lerp(np.asarray(state["row_var"], np.float64), np.mean(g * g, -1, keepdims=True), w)
        col = lerp(np.asarray(state["col_var"], np.float64), np.mean(g * g, -2, keepdims=True), w)
        v = row * col / np.maximum(np.mean(row, -2, keepdims=True), eps1)
        new = {"row_var": row, "col_var": col}
    else:
        v = lerp(np.asarray(state["variance"], np.float64), g * g, w)
        new = {"variance": v}
    u = g / np.sqrt(np.maximum(v, eps1 * eps1))
    denom = max(1.0, np.sqrt(np.sum(u * u)) / (np.sqrt(u.size) * d))
    delta = (-alpha / denom) * u
    return p + delta, new, delta


def zero_state(shape):
    if len(shape) < 2:
        return {"variance": np.zeros(shape)}
    return {"row_var": np.zeros(shape[:-1] + (1,)), "col_var": np.zeros(shape[:-2] + (1, shape[-1]))}
