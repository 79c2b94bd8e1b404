"""zero_amd.optim.NorMuon behind the ZeRO-1/2 ShardedOptimizer, modelled on the Muon optimizer test
(whose inputs and helpers it shares): the trajectory against a float64 oracle with the class's own
fp32 CPU step as the yardstick, world sizes 2 and 3 against world size 1 bit for bit (the row second
moments included), a checkpoint, and the refusals."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _normuon_oracle as no
from _zero_run import init_pg, module_for, spawn_batch
from conftest import free_port
from test_gpu_muon_optimizer import REFUSED, SPLIT, _bits, _inputs, _master, _step, pg1  # noqa: F401

pytestmark = pytest.mark.gpu

GROUPS = [dict(lr=0.02, weight_decay=0.1, nesterov=True, momentum=0.95),
          dict(lr=0.01, weight_decay=0.05, nesterov=False, momentum=0.3, beta2=0.9, norm_eps=1e-6)]


def _normuon(params):
    from zero_amd.optim import NorMuon

    return NorMuon([dict(params=params[:SPLIT], **GROUPS[0]), dict(params=params[SPLIT:], **GROUPS[1])])


def _make(variant, init, dev, dtype=torch.float32, **kw):
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dtype).to(dev)) for a in init]
    return params, module_for(variant).ShardedOptimizer(_normuon(params), **kw)


def _rows(opt, params):
    """The row second moments this rank holds (its owned matrices), as bits."""
    return {i: opt.optimizer.state[p]["row_exp_avg_sq"].cpu().view(torch.int32).numpy().copy()
            for i, p in enumerate(params) if "row_exp_avg_sq" in opt.optimizer.state[p]}


@pytest.mark.parametrize("variant,dtype", [(1, torch.float32), (2, torch.float32), (2, torch.bfloat16)])
def test_trajectory_against_float64_oracle(gpu, pg1, variant, dtype):  # noqa: F811
    init, grads = _inputs(3, dtype)
    ref = [a.astype(np.float64) for a in init]
    rbuf, rv = [np.zeros_like(a) for a in ref], [np.zeros(a.shape[0]) for a in ref]
    cpu = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
    cpu_opt = _normuon(cpu)
    params, opt = _make(variant, init, gpu, dtype)
    for t, step in enumerate(grads):
        _step(opt, params, step, gpu)
        for q, g in zip(cpu, step):
            q.grad = torch.from_numpy(g.copy())
        cpu_opt.step()
        for i, g in enumerate(step):
            ref[i], rbuf[i], rv[i] = no.step(ref[i], g.astype(np.float64), rbuf[i], rv[i], **GROUPS[i >= SPLIT])
            ours = np.linalg.norm(_master(opt, params[i]) - ref[i])
            theirs = np.linalg.norm(cpu[i].detach().double().numpy() - ref[i])
            print(f"step {t} param {i}: ours {ours:.3e}, class fp32 {theirs:.3e}, ratio {ours / theirs:.3f}")
            assert ours <= 1.5 * theirs
            st = opt.optimizer.state[params[i]]
            assert set(st) >= {"momentum_buffer", "row_exp_avg_sq"} and "step" not in st
            v = st["row_exp_avg_sq"]  # a live fp32 view, one per row, moved by this step
            assert v.shape == (params[i].shape[0],) and v.dtype == torch.float32 and bool((v > 0).all())


def test_checkpoint_continues_bit_for_bit(gpu, pg1):  # noqa: F811
    init, grads = _inputs(4, torch.bfloat16)
    params, opt = _make(2, init, gpu, torch.bfloat16)
    for step in grads:
        _step(opt, params, step, gpu)
    pa, oa = _make(2, init, gpu, torch.bfloat16)
    for step in grads[:2]:
        _step(oa, pa, step, gpu)
    sd = oa.state_dict()
    assert set(sd["state"][0]) == {"momentum_buffer", "row_exp_avg_sq", "master_residual"}
    pb, ob = _make(2, [p.detach().float().cpu().numpy() for p in pa], gpu, torch.bfloat16)
    ob.load_state_dict(sd)
    for step in grads[2:]:
        _step(ob, pb, step, gpu)
    assert all(np.array_equal(_master(ob, p), _master(opt, q)) for p, q in zip(pb, params))
    assert all(np.array_equal(a, b) for a, b in zip(_rows(ob, pb).values(), _rows(opt, params).values()))


def _ws_worker(rank, ws, port, want):
    """Identical gradients on every rank: the world-size-1 run's parameters and rows, bit for bit."""
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
        rows = _rows(opt, params)
        assert sorted(rows) == sorted(int(i) for i in opt.engine.owned_param_indices())
        assert all(np.array_equal(v, want[t][1][i]) for i, v in rows.items()), (ws, rank, t)
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
            want.append((_bits(params), _rows(opt, params)))
    finally:
        dist.destroy_process_group()
    del opt, params
    spawn_batch(ws, [(_ws_worker, (want,))])


@pytest.mark.parametrize("variant,kw", REFUSED)
def test_unsupported_combinations_are_refused_at_construction(gpu, pg1, variant, kw):  # noqa: F811
    from zero_amd._update import check_muon

    init, _ = _inputs(0)
    with pytest.raises(ValueError, match="NorMuon"):
        if kw == "carry":  # ZeRO-1 at world size > 1: what the constructor passes there
            check_muon(carry=True, kind="normuon")
        else:
            _make(variant, init, gpu, **kw)
