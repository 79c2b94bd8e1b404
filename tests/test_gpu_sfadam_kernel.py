"""The fused Schedule-Free AdamW kernels (SfAdamRule through the update kernel pair, the two swap
kernels) through zero_amd.kernels.SfAdamSet: 3 steps with c = 1, 0.8, 0.444 (both forms of the
lerp), the swap to x and back, every array the kernels may write compared whole (gaps and 4,096
elements of slack included) and bit for bit with tests/_sfadam_oracle.py.  Kinds as
tests/test_gpu_lion_kernel.py; the swap writes the bf16 copy alone beside an fp32 master ("bf16")
and is in place where the parameter is (half of) its own master ("f32", the split master).
"""
import numpy as np
import pytest
import torch

import _sfadam_oracle as so
from oracle import c_oracle
from test_gpu_lion_kernel import CHUNK, KINDS, SLACK, TIES

pytestmark = pytest.mark.gpu

C = CHUNK["split"]  # 4,096; (elements, offset from a 16-byte boundary): one starts 4 B off
LENGTHS = [(1, 0), (63, 0), (C - 1, 0), (C, 0), (C + 1, 1), (2 * C + 5, 0)]
HP = dict(beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.1)
SCHED = so.schedule(2.5e-3, 3, warmup_steps=2)
CASES = [(k, {}) for k in KINDS] + [("split", dict(coef=0.25)),
                                    ("f32", dict(grad_div=2.0, maximize=True))]
SEGS, _off = [], 0
for _n, _shift in LENGTHS:
    _off = (_off + 3) // 4 * 4 + _shift
    SEGS.append((_off, _n))
    _off += _n
N = _off + SLACK


def _inputs(kind):
    """Arrays by name and the gradients; split-encoding ties and a 0 / 0 element head long segments."""
    rng = np.random.default_rng(41)
    master = (rng.standard_normal(N) * 0.02).astype(np.float32)
    z = master + rng.standard_normal(N).astype(np.float32) * np.float32(1e-3)
    v = (rng.standard_normal(N) ** 2 * 1e-4).astype(np.float32)
    grads = [(rng.standard_normal(N) * 1e-2).astype(np.float32) for _ in SCHED]
    for o, n in SEGS:
        if n >= 16:
            master.view(np.uint32)[o:o + len(TIES)] = TIES
            for a in [v] + grads:
                a[o + 12] = 0.0
    if kind in ("split", "bf16"):
        grads = [so.f32_to_bf16_bits(g) for g in grads]
    A = {"z": z, "v": v}
    if kind in ("split", "f32split"):
        A["hi"], A["lo"] = c_oracle.split_master(master)
    else:
        A["p"] = master
    if kind == "bf16":
        A["pb"] = np.zeros(N, np.uint16)
    return A, grads


def _reference(kind, coef=None, **hpk):
    """[after the steps, after eval, after train] as copies of the arrays."""
    A, grads = _inputs(kind)
    split, stages = "hi" in A, []
    for stage in range(3):
        for o, n in SEGS:
            s = slice(o, o + n)
            y = c_oracle.join_master(A["hi"][s], A["lo"][s]) if split else A["p"][s]
            if stage == 0:
                for g, (t, lr_t, c) in zip(grads, SCHED):
                    hp = so.SfHP(lr_t, step=t, c=c, **HP, **hpk)
                    y, A["z"][s], A["v"][s] = so.sfadam_elem(g[s], y, A["z"][s], A["v"][s], hp,
                                                             coef=coef)
                x = y
            else:
                x = so.swap(y, A["z"][s], HP["beta1"], stage == 1)
            if split:
                A["hi"][s], A["lo"][s] = c_oracle.split_master(x)
            elif kind == "bf16":  # the copy alone shows x: eval rounds x, train the master again
                A["p"][s], A["pb"][s] = y, so.f32_to_bf16_bits(x if stage < 2 else y)
            else:
                A["p"][s] = x
        stages.append({k: a.copy() for k, a in A.items()})
    return stages


def _run_gpu(gpu, kind, coef=None, **hpk):
    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
    from zero_amd.kernels import SfAdamSet, sfadam_hparams

    A, grads = _inputs(kind)
    split, g32 = "hi" in A, kind in ("f32", "f32split")
    dev = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)  # noqa: E731
    T = {k: dev(a) for k, a in A.items()}
    G = torch.zeros(N, dtype=torch.float32 if g32 else torch.int16, device=gpu)
    at = lambda k, o: T[k].data_ptr() + o * T[k].element_size() if k in T else 0  # noqa: E731
    rows = []
    for o, n in SEGS:
        assert 0 <= o and o + n <= N - SLACK  # every segment inside the arrays
        mst = [at("hi", o), at("lo", o), at("hi", o)] if split else [at("p", o), at("p", o), at("pb", o)]
        rows.append([G.data_ptr() + o * G.element_size()] + mst + [at("z", o), at("v", o), 0, 0, n])
    sset = SfAdamSet(np.array(rows, np.uint64), ZS_F32 if g32 else ZS_BF16,
                     ZS_BF16_SPLIT if split else ZS_BF16, wide_grads=g32)
    cdev = None if coef is None else torch.tensor([coef], dtype=torch.float32, device=gpu)
    st = torch.cuda.current_stream()
    for g, (t, lr_t, c) in zip(grads, SCHED):
        G.copy_(dev(g))
        sset.run(sfadam_hparams(lr_t, HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"], t, c,
                                **hpk), st, coef=cdev)
    stages = [{k: a.cpu().numpy() for k, a in T.items()}]
    for weight, to_eval in ((1 - 1 / HP["beta1"], True), (1 - HP["beta1"], False)):
        sset.swap(weight, to_eval, st)
        stages.append({k: a.cpu().numpy() for k, a in T.items()})
    return stages


@pytest.mark.parametrize("kind,kw", CASES, ids=lambda x: x if isinstance(x, str) else "-".join(x))
def test_steps_and_swap_equal_the_oracle(gpu, kind, kw):
    want, got = _reference(kind, **kw), _run_gpu(gpu, kind, **kw)
    for stage, w, g in zip(("steps", "eval", "train"), want, got):
        assert set(w) == set(g)
        for name in w:
            bad = np.flatnonzero(g[name].view(np.uint8) != w[name].view(np.uint8))
            assert bad.size == 0, f"{stage}, {name}: bytes differ from the oracle, first at {bad[:8]}"
