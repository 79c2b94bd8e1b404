"""Fused LAMB at the kernel level, one set built directly over the ABI: pass L1
(zs_lambset_run_moments), the per-parameter reduction and the finishing kernel (zs_lamb_finish;
``LambSetStage``) and pass L2 (zs_lambset_run_apply) against tests/_lamb_oracle.py.

Segments, with C the chunk (4,096 split master, 2,048 fp32 master): 1, 3, C - 1, C, C + 5 and
3C + 1027 elements, one parameter spread over two entries, one entry that starts one element off
the 16-byte alignment (the scalar kernel takes all of it), and three edge parameters: all-zero
weights, a zero gradient, an entry without a gradient.

The bound on a norm: a lane adds k = 4 * adam_groups fp32 terms per chunk, one fma rounding each;
everything above the lane is double; then one rounding each for the sum and the root: (k + 2) * 2^-24
relative to the float64 norm of the same fp32 values.  -s adds the division and the product:
(k + 4) * 2^-24.
"""
import numpy as np
import pytest

import _lamb_oracle as lo
from oracle import c_oracle
from oracle import zero_oracle as zo

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, U = 2e-3, (0.9, 0.999), 1e-6, 2.0 ** -24
ZERO_W, ZERO_G, NO_G, N_PAR = 7, 8, 9, 11  # the edge parameters; parameters in all


def _segments(C):
    """[(offset, n, parameter)]: offsets 8-element aligned but for the shifted entry."""
    lens = [(1, 0), (3, 1), (C - 1, 2), (C, 3), (C + 5, 4), (3 * C + 1027, 5), (C + 8, 6), (520, 6),
            (300, ZERO_W), (C + 3, ZERO_G), (C + 3, NO_G)]
    segs, o = [], 0
    for n, par in lens:
        segs.append((o, n, par))
        o = (o + n + 7) // 8 * 8
    segs.append((o + 1, 777, 10))  # off 16-byte (fp32) and 8-byte (bf16) alignment
    return segs, o + 1 + 777 + 64


def _same(t, ref):
    return np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(ref).view(np.uint8))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("g32", [False, True])
def test_two_steps(gpu, g32, split, clip):
    import torch

    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
    from zero_amd._update import LambSetStage
    from zero_amd.kernels import AdamSet, adam_groups, lamb_hparams

    k = 4 * adam_groups(split)
    segs, N = _segments(256 * k)
    rng = np.random.default_rng(11 + 2 * g32 + split)
    P = rng.standard_normal(N).astype(np.float32)
    M, V = np.zeros(N, np.float32), np.zeros(N, np.float32)
    for o, n, par in segs:
        if par == ZERO_W:
            P[o:o + n] = 0
    if split:  # (as the two words will hold it)
        P = c_oracle.join_master(*c_oracle.split_master(P))
    wd =0.01 if clip else 0.0  # (wd == 0: the zero gradient gives ‖u‖ == 0)
    coef = np.float32(0.37) if clip else None
    coef_d = torch.tensor([0.37], device=gpu) if clip else None
    host = dict(zip(("a", "b"), c_oracle.split_master(P))) if split else \
        {"a": P, "b": zo.f32_to_bf16_bits(P)}  # split: hi, lo; else the fp32 master, its bf16 copy
    dev = {name: torch.from_numpy(np.ascontiguousarray(x).view(np.int16 if x.dtype == np.uint16
                                                               else x.dtype).copy()).to(gpu)
           for name, x in {**host, "m": M, "v": V}.items()}
    G = torch.zeros(N, dtype=torch.float32 if g32 else torch.int16, device=gpu)
    at = lambda t, o: t.data_ptr() + o * t.element_size()  # noqa: E731
    a, b = dev["a"], dev["b"]
    rows = [[0 if par == NO_G else at(G, o), at(a, o), at(b if split else a, o),
             at(a if split else b, o), at(dev["m"], o), at(dev["v"], o), 0, 0, n] for o, n, par in segs]
    aset = AdamSet(np.array(rows, np.uint64), ZS_F32 if g32 else ZS_BF16,
                   ZS_BF16_SPLIT if split else ZS_BF16, wide_grads=g32 and split)
    stage = LambSetStage(aset, [par for _, _, par in segs], N_PAR, LR, gpu, fill=-7.0)
    st = torch.cuda.current_stream()
    idx_of = {par: np.concatenate([np.arange(o, o + n) for o, n, q in segs if q == par])
              for par in range(N_PAR) if par != NO_G}

    def state_same():  # m, v and the master as stored (the entry without a gradient included)
        if split:
            hi, lo_ = c_oracle.split_master(P)
            return _same(dev["m"], M) and _same(dev["v"], V) and _same(a, hi) and _same(b, lo_)
        return _same(dev["m"], M) and _same(dev["v"], V) and _same(a, P)

    for t in (1, 2):
        g = (rng.standard_normal(N) * 10.0 ** rng.integers(-4, 1, N)).astype(np.float32)
        g[idx_of[ZERO_G]] = 0
        if not g32:
            gb = zo.f32_to_bf16_bits(g)
            g = (gb.astype(np.uint32) << 16).view(np.float32)
        G.copy_(torch.from_numpy(g if g32 else gb.view(np.int16)).to(gpu))
        gd = 3.0 if clip else 2.0
        hp = lamb_hparams(*BETAS, EPS, wd, t, grad_div=gd)
        ohp = lo.LambHP(LR, *BETAS, EPS, wd, t, grad_div=gd)
        # L1: the moments move, the parameter does not; every slot is written
        aset.run_lamb_moments(hp, stage.partials, st, coef=coef_d)
        exp = {}
        for par, idx in idx_of.items():
            _, M[idx], V[idx], _, exp[par] = lo.step(P[idx], g[idx], M[idx], V[idx], ohp, coef=coef,
                                                     norms64=True)
        assert state_same() and not bool((stage.partials == -7.0).any())
        # the norms, the ratios and -s
        stage.finish(st)
        wn_k, un_k = stage.norms2.cpu().numpy().reshape(2, N_PAR)
        r_k, ns_k = stage.ratios.cpu().numpy(), stage.neg_s.cpu().numpy()
        for par, (wn, un, _, ns) in exp.items():
            assert abs(float(wn_k[par]) - wn) <= (k + 2) * U * wn
            assert abs(float(un_k[par]) - un) <= (k + 2) * U * un
            assert abs(float(ns_k[par]) - ns) <= (k + 4) * U * abs(ns)
        assert r_k[NO_G] == 1.0 and (t > 1 or r_k[ZERO_W] == 1.0)  # (step 1 moved the zeros)
        assert wd != 0.0 or (un_k[ZERO_G] == 0.0 and r_k[ZERO_G] == 1.0)
        # L2 with the kernel's own -s
        aset.run_lamb_apply(hp, stage.neg_s, st)
        for par, idx in idx_of.items():
            u = lo.direction(P[idx], M[idx], V[idx], ohp)
            P[idx] = lo.fma32(np.full_like(u, ns_k[par]), u, P[idx])
        assert state_same()
        if split:  # (the residual int16 cannot hold, +0x8000, moves the stored master 1 ulp)
            P = c_oracle.join_master(*c_oracle.split_master(P))
        else:  # (b started as the bf16 of P everywhere: the untouched entry's copy is compared too)
            assert _same(b, zo.f32_to_bf16_bits(P))
