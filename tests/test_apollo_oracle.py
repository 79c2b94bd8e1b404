"""zero_amd.optim.Apollo on the CPU: its sign matrix against the library's own generator, its fp32
step against the float64 oracle, and when sigma is re-drawn."""
import ctypes

import numpy as np
import pytest
import torch

import _apollo_oracle as ao

U = 2.0 ** -24
HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, scale=2.0, norm_growth=1.01)


@pytest.mark.parametrize("seed,epoch", [(0, 0), (7, 3), ((5 << 32) + 1, (1 << 33) + 2)])
def test_sigma_is_the_librarys_bits(seed, epoch):
    from zero_amd import _lib
    from zero_amd.optim import apollo_sigma

    k0, k1, r = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    _lib.call("zs_sr_keys", seed, epoch, ctypes.byref(k0), ctypes.byref(k1))
    K, rank = 72, 5
    want = np.empty((K, rank))
    for k in range(K):
        for j in range(rank):
            _lib.call("zs_sr_bits", (j << 32) | (k >> 5), k0.value, k1.value, ctypes.byref(r))
            want[k, j] = 1 - 2 * ((r.value >> (k & 31)) & 1)
    assert np.array_equal(ao.sigma(K, rank, seed, epoch), want)
    assert np.array_equal(apollo_sigma(K, rank, seed, epoch), want)


@pytest.mark.parametrize("shape,rank,scale_type", [((37, 53), 16, "channel"), ((64, 24), 1, "tensor")])
def test_fp32_step_stays_near_float64(shape, rank, scale_type):
    """Four steps, update_proj_gap=2.  Bound per step on |p - p64|, relative to |a_c g|: the fp32
    sketch is a K-term sum in any order (K u of sum |g|, at most K sqrt(K) u of |S| for these
    normal gradients, taken as K^1.5), which enters s_c twice (Nh and S) through moments that
    remember it, plus the 29 u of the element-wise pieces (tests/test_gpu_apollo_kernel.py) and the
    step's own fma: (2 K^1.5 + 30) u per step, and the steps add: 4 of them."""
    from zero_amd.optim import Apollo

    rng = np.random.default_rng(0)
    p = torch.nn.Parameter(torch.from_numpy((rng.standard_normal(shape) * 0.05).astype(np.float32)))
    opt = Apollo([p], HP["lr"], (HP["beta1"], HP["beta2"]), HP["eps"], HP["weight_decay"], rank=rank,
                 scale=HP["scale"], scale_type=scale_type, update_proj_gap=2, seed=3)
    ref, M, V, F = p.detach().double().numpy(), np.zeros((max(shape), rank)), np.zeros((max(shape), rank)), 0.0
    K, moved = min(shape), 0.0
    for t in range(1, 5):
        g = (rng.standard_normal(shape) * 1e-2).astype(np.float32)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        new, M, V, F = ao.step(ref, g.astype(np.float64), M, V, F, t, seed=3, rank=rank, update_proj_gap=2,
                               scale_type=scale_type, **HP)
        moved += np.abs(new - ref * (1 - HP["lr"] * HP["weight_decay"])).max()
        ref = new
        err = np.abs(p.detach().double().numpy() - ref).max()
        bound = (2 * K ** 1.5 + 30) * U * moved + t * U * np.abs(ref).max()
        print(f"t={t}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert abs(float(opt.state[p]["scaled_grad_norm"]) - F) <= (K ** 1.5 + 30) * U * F


def test_sigma_is_redrawn_at_steps_3_and_5_and_differs_between_parameters():
    from zero_amd.optim import Apollo, apollo_sigma

    ps = [torch.nn.Parameter(torch.zeros(8, 40)), torch.nn.Parameter(torch.zeros(8, 40))]
    opt = Apollo(ps, rank=4, update_proj_gap=2, betas=(0.0, 0.999), seed=11)
    g, seen = torch.ones(8, 40), []
    for t in range(1, 6):
        for p in ps:
            p.grad = g.clone()
        opt.step()
        # beta1 = 0 and a gradient of ones: exp_avg is the column sums of sigma / sqrt(rank)
        seen.append([opt.state[p]["exp_avg"][0].numpy().copy() for p in ps])
        for q, x in enumerate(seen[-1]):
            assert np.array_equal(x * 2, apollo_sigma(8, 4, 11 + q, (t - 1) // 2).sum(0))
    same = [np.array_equal(a[0], b[0]) for a, b in zip(seen, seen[1:])]
    assert same == [True, False, True, False]
    assert not np.array_equal(apollo_sigma(8, 4, 11, 0), apollo_sigma(8, 4, 12, 0))
    assert [int(opt.state[p]["seed"]) for p in ps] == [11, 12]
