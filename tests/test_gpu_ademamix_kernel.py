"""The fused AdEMAMix kernels through AdEMAMixSet: two steps inside both warm-ups, every array
compared whole (a 64-element border in front, the gaps, 4,096 elements of slack behind) and bit for
bit with tests/_ademamix_oracle.py, the master too.  Kinds as tests/test_gpu_lion_kernel.py."""
import numpy as np
import pytest
import torch

import _ademamix_oracle as ao
from oracle import c_oracle
from test_gpu_lion_kernel import CHUNK, KINDS, SLACK, TIES, _layout, _tune
from zero_amd.optim import ademamix_schedule

pytestmark = pytest.mark.gpu

HP = dict(lr=1e-2, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.1)
SCHED = [ademamix_schedule(t, 5.0, 0.9, 0.999, alpha_warmup=3, beta3_warmup=3) for t in (1, 2)]
CASES = [(k, {}) for k in KINDS] + [("split", dict(coef=0.25)), ("f32", dict(coef=0.25, maximize=True)),
                                    ("split", dict(carry=True, grad_div=2.0, carry_mul=1.0)),
                                    ("bf16", dict(carry=True, grad_div=3.0, carry_mul=2.0)),
                                    ("split", dict(many=True))]


def _segs(kind, many):
    """C+1 lies 4 bytes off a 16-byte boundary (the scalar kernel); ``many``: 300 chunks + 5."""
    C = CHUNK[kind]
    spec = [(300 * C + 5, True, 0)] if many else \
        [(1, True, 0), (3, True, 0), (C - 1, True, 0), (C, True, 0), (C + 1, True, 1),
         (257, False, 0), (2 * C + 5, True, 0)]
    segs = [(o + 64, n, has_g) for o, n, has_g in _layout(spec)]
    return segs, segs[-1][0] + segs[-1][1] + SLACK


def _inputs(kind, segs, N, carry):
    rng = np.random.default_rng(43)
    master = (rng.standard_normal(N) * 0.02).astype(np.float32)
    A = {k: (rng.standard_normal(N) * 5e-3).astype(np.float32) for k in ("m1", "m2")}
    A["v"] = (rng.standard_normal(N) ** 2 * 1e-4).astype(np.float32)
    grads = [(rng.standard_normal(N) * 1e-2).astype(np.float32) for _ in SCHED]
    for o, n, _ in segs:  # split-encoding ties and a 0 / 0 element head the long segments
        if n >= 16:
            master.view(np.uint32)[o:o + len(TIES)] = TIES
            for a in list(A.values()) + grads:
                a[o + 12] = 0.0
    if kind in ("split", "bf16"):
        grads = [ao.f32_to_bf16_bits(g) for g in grads]
    if carry:
        A["carry"] = (rng.standard_normal(N) * 1e-2).astype(np.float32)
    if kind in ("split", "f32split"):
        A["hi"], A["lo"] = c_oracle.split_master(master)
    else:
        A["p"] = master
    if kind == "bf16":
        A["pb"] = np.zeros(N, np.uint16)
    return A, grads


def _reference(kind, segs, A, grads, coef=None, carry=False, **hpk):
    for t, (g, (a_t, b3_t)) in enumerate(zip(grads, SCHED), 1):
        hp = ao.MixHP(HP["lr"], HP["beta1"], HP["beta2"], b3_t, a_t, HP["eps"], HP["weight_decay"], t, **hpk)
        for o, n, has_g in segs:
            s = slice(o, o + n)
            p = c_oracle.join_master(A["hi"][s], A["lo"][s]) if "hi" in A else A["p"][s]
            out = ao.ademamix_elem(g[s] if has_g else np.zeros(n, np.float32), p, A["m1"][s], A["m2"][s],
                                   A["v"][s], hp, coef=coef, carry=A["carry"][s] if carry else None)
            p, A["m1"][s], A["m2"][s], A["v"][s] = out[:4]
            if carry:
                A["carry"][s] = out[4]
            if "hi" in A:
                A["hi"][s], A["lo"][s] = c_oracle.split_master(p)
            else:
                A["p"][s] = p
            if kind == "bf16":
                A["pb"][s] = ao.f32_to_bf16_bits(p)
    return A


def _run_gpu(gpu, kind, segs, A, grads, coef=None, carry=False, **hpk):
    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
    from zero_amd.kernels import AdEMAMixSet, ademamix_hparams

    split, g32 = "hi" in A, kind in ("f32", "f32split")
    dev = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)  # noqa: E731
    T = {k: dev(a) for k, a in A.items()}
    G = torch.zeros(len(A["v"]), dtype=torch.float32 if g32 else torch.int16, device=gpu)
    at = lambda k, o: T[k].data_ptr() + o * T[k].element_size() if k in T else 0  # noqa: E731
    rows = []
    for o, n, has_g in segs:
        assert 64 <= o and o + n <= len(A["v"]) - SLACK  # every segment inside the arrays
        mst = [at("hi", o), at("lo", o), at("hi", o)] if split else [at("p", o), at("p", o), at("pb", o)]
        rows.append([G.data_ptr() + o * G.element_size() if has_g else 0] + mst +
                    [at("m1", o), at("v", o), at("m2", o), at("carry", o), n])
    mset = AdEMAMixSet(np.array(rows, np.uint64), ZS_F32 if g32 else ZS_BF16,
                       ZS_BF16_SPLIT if split else ZS_BF16, wide_grads=g32)
    cdev = None if coef is None else torch.tensor([coef], dtype=torch.float32, device=gpu)
    st = torch.cuda.current_stream()
    for t, (g, (a_t, b3_t)) in enumerate(zip(grads, SCHED), 1):
        G.copy_(dev(g))
        mset.run(ademamix_hparams(HP["lr"], HP["beta1"], HP["beta2"], b3_t, a_t, HP["eps"],
                                  HP["weight_decay"], t, **hpk), st, coef=cdev)
    return {k: a.cpu().numpy() for k, a in T.items()}


@pytest.mark.parametrize("kind,kw", CASES, ids=lambda x: x if isinstance(x, str) else "-".join(x))
def test_two_steps_equal_the_oracle(gpu, kind, kw):
    kw = dict(kw)
    many = kw.pop("many", False)
    segs, N = _segs(kind, many)
    (A, grads), (B, _) = (_inputs(kind, segs, N, kw.get("carry", False)) for _ in range(2))
    want = _reference(kind, segs, A, grads, **kw)
    if many:  # one workgroup per CU: every workgroup walks several chunks
        _tune(b"adam_wg_per_cu", 1)
    try:
        got = _run_gpu(gpu, kind, segs, B, grads, **kw)
    finally:
        _tune(b"adam_wg_per_cu", 0)
    for name in want:
        bad = np.flatnonzero(got[name].view(np.uint8) != want[name].view(np.uint8))
        assert bad.size == 0, f"{name}: bytes differ from the oracle, first at {bad[:8]}"
