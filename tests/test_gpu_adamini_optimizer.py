"""zero_amd.optim.AdamMini behind the ZeRO-1/2 ShardedOptimizer, in the form of the NorMuon optimizer
test: the trajectory against a float64 oracle with the class's own fp32 CPU step as the yardstick,
world sizes 2 and 3 against world size 1 bit for bit (block_exp_avg_sq included), a checkpoint, and
a parameter without a gradient."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _adamini_oracle as ao
from _zero_run import init_pg, module_for, spawn_batch
from conftest import free_port
from test_gpu_muon_optimizer import _bits, _step, pg1  # noqa: F401

pytestmark = pytest.mark.gpu

# a 2-D with block_rows=1, a 1-D | a 2-D with block_rows=2, a 3-D (rows of 9 * 16 elements)
SHAPES = [(37, 53), (24,), (70, 8), (4, 9, 16)]
SPLIT = 2  # parameters [0, SPLIT) are group 0
GROUPS = [dict(lr=1e-2, weight_decay=0.1), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, block_rows=2)]
KW = [dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1),
      dict(lr=3e-3, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.0)]
BR = [1, 1, 2, 2]


def _inputs(steps, dtype=torch.float32, short=False):
    rng = np.random.default_rng(3)
    rnd = lambda a, dt: torch.from_numpy(a.astype(np.float32)).to(dt).float().numpy()  # noqa: E731
    init = [rnd(rng.standard_normal(s) * 0.05, dtype) for s in SHAPES]
    gd = torch.bfloat16 if short else dtype  # (8 significant bits: the sum over ranks / ws is exact)
    return init, [[rnd(rng.standard_normal(s) * 1e-2, gd) for s in SHAPES] for _ in range(steps)]


def _adamini(params):
    from zero_amd.optim import AdamMini

    return AdamMini([dict(params=params[:SPLIT], **GROUPS[0]), dict(params=params[SPLIT:], **GROUPS[1])])


def _make(variant, init, dev, dtype=torch.float32, **kw):
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dtype).to(dev)) for a in init]
    return params, module_for(variant).ShardedOptimizer(_adamini(params), **kw)


def _master(opt, p):
    from zero_amd._update import join_split_master

    st = opt.optimizer.state[p]
    w = st["master_param"] if "master_param" in st else \
        join_split_master(p, st["master_residual"]) if "master_residual" in st else p
    return w.detach().cpu().double().numpy()


def _blocks(opt, params):
    """The block second moments this rank holds (its owned parameters), as bits."""
    return {i: opt.optimizer.state[p]["block_exp_avg_sq"].cpu().view(torch.int32).numpy().copy()
            for i, p in enumerate(params) if "block_exp_avg_sq" in opt.optimizer.state[p]}


@pytest.mark.parametrize("variant,dtype,master", [(1, torch.float32, "split"), (2, torch.float32, "split"),
                                                  (2, torch.bfloat16, "split"), (2, torch.bfloat16, "fp32")])
def test_trajectory_against_float64_oracle(gpu, pg1, variant, dtype, master):  # noqa: F811
    init, grads = _inputs(3, dtype)
    ref = [a.astype(np.float64) for a in init]
    rm = [np.zeros_like(a) for a in ref]
    rv = [np.zeros(ao.blocks(s, b)) for s, b in zip(SHAPES, BR)]
    cpu = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
    cpu_opt = _adamini(cpu)
    params, opt = _make(variant, init, gpu, dtype, master=master)
    for t, step in enumerate(grads):
        _step(opt, params, step, gpu)
        for q, g in zip(cpu, step):
            q.grad = torch.from_numpy(g.copy())
        cpu_opt.step()
        for i, g in enumerate(step):
            ref[i], rm[i], rv[i], _ = ao.step(ref[i], g.astype(np.float64), rm[i], rv[i], t + 1, rv[i].size,
                                              **KW[i >= SPLIT])
            ours = np.linalg.norm(_master(opt, params[i]) - ref[i])
            theirs = np.linalg.norm(cpu[i].detach().double().numpy() - ref[i])
            print(f"step {t} param {i}: ours {ours:.3e}, class fp32 {theirs:.3e}, ratio {ours / theirs:.3f}")
            assert ours <= 1.5 * theirs
            st = opt.optimizer.state[params[i]]
            assert float(st["step"]) == t + 1 and st["exp_avg"].shape == params[i].shape
            v = st["block_exp_avg_sq"]  # a live fp32 view, one per block, moved by this step
            assert v.shape == rv[i].shape and v.dtype == torch.float32 and bool((v > 0).all())


def test_checkpoint_continues_bit_for_bit(gpu, pg1):  # noqa: F811
    init, grads = _inputs(4, torch.bfloat16)
    params, opt = _make(2, init, gpu, torch.bfloat16)
    for step in grads:
        _step(opt, params, step, gpu)
    pa, oa = _make(2, init, gpu, torch.bfloat16)
    for step in grads[:2]:
        _step(oa, pa, step, gpu)
    sd = oa.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "block_exp_avg_sq", "master_residual"}
    pb, ob = _make(2, [p.detach().float().cpu().numpy() for p in pa], gpu, torch.bfloat16)
    ob.load_state_dict(sd)
    for step in grads[2:]:
        _step(ob, pb, step, gpu)
    assert all(np.array_equal(_master(ob, p), _master(opt, q)) for p, q in zip(pb, params))
    assert all(np.array_equal(a, b) for a, b in zip(_blocks(ob, pb).values(), _blocks(opt, params).values()))


def test_a_parameter_without_gradient_keeps_state_and_step(gpu, pg1):  # noqa: F811
    from _zero_run import set_grad

    init, grads = _inputs(2)
    params, opt = _make(2, init, gpu)
    _step(opt, params, grads[0], gpu)
    st = opt.optimizer.state[params[2]]
    before = (params[2].detach().clone(), st["exp_avg"].clone(), st["block_exp_avg_sq"].clone())
    opt.zero_grad()
    for i, (p, g) in enumerate(zip(params, grads[1])):
        if i != 2:
            set_grad(p, torch.from_numpy(g.copy()).to(gpu))
    opt.step()
    st = opt.optimizer.state[params[2]]
    assert float(st["step"]) == 1 and float(opt.optimizer.state[params[0]]["step"]) == 2
    assert all(torch.equal(a, b) for a, b in zip(before, (params[2].detach(), st["exp_avg"], st["block_exp_avg_sq"])))


def _ws_worker(rank, ws, port, want):
    """Identical gradients on every rank: the world-size-1 run's parameters and blocks, bit for bit."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    init_pg(rank, ws, port)
    init, grads = _inputs(2, short=True)
    params, opt = _make(2, init, dev, comm=test_comm(), bucket_mb=ws * 64 * 4 / (1 << 20))
    for t, step in enumerate(grads):
        _step(opt, params, step, dev)
        torch.cuda.synchronize()
        for i, (got, exp) in enumerate(zip(_bits(params), want[t][0])):
            assert np.array_equal(got, exp), (ws, rank, t, i)
        blocks = _blocks(opt, params)
        assert sorted(blocks) == sorted(int(i) for i in opt.engine.owned_param_indices())
        assert all(np.array_equal(v, want[t][1][i]) for i, v in blocks.items()), (ws, rank, t)
    dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_world_sizes_match_world_size_one(gpu, ws):
    init, grads = _inputs(2, short=True)
    init_pg(0, 1, free_port())
    try:
        params, opt = _make(2, init, gpu)
        want = []
        for step in grads:
            _step(opt, params, step, gpu)
            want.append((_bits(params), _blocks(opt, params)))
    finally:
        dist.destroy_process_group()
    del opt, params
    spawn_batch(ws, [(_ws_worker, (want,))])
