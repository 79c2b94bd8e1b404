"""torch.optim.Muon behind the ZeRO-1/2 ShardedOptimizer: the trajectory against a float64 oracle
with torch's own fp32 CPU run as the yardstick, world sizes 2 and 3 against world size 1 bit for
bit, checkpoints, a second ShardedOptimizer over the rest of the model, and the refusals."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _muon_oracle as mo
from _zero_run import init_pg, module_for, set_grad, spawn_batch
from conftest import free_port

pytestmark = pytest.mark.gpu

SHAPES = [(33, 70), (96, 40), (33, 70), (130, 257)]
SPLIT = 2  # parameters [0, SPLIT) are group 0
GROUPS = [dict(lr=0.02, weight_decay=0.1, nesterov=True, momentum=0.95),
          dict(lr=0.01, weight_decay=0.05, nesterov=False, momentum=0.3, adjust_lr_fn="match_rms_adamw")]


@pytest.fixture
def pg1():
    init_pg(0, 1, free_port())
    yield
    dist.destroy_process_group()

def _inputs(steps, dtype=torch.float32, seed=3, short=False):
    """Start and gradients as fp32 arrays holding ``dtype`` values; ``short``: gradients with 8
    significant bits, so the sum over 2 or 3 ranks and its division by the world size are exact."""
    rng = np.random.default_rng(seed)
    rnd = lambda a: torch.from_numpy(a.astype(np.float32)).to(dtype).float().numpy()  # noqa: E731
    init = [rnd(rng.standard_normal(s) * 0.05) for s in SHAPES]
    gd = torch.bfloat16 if short else dtype
    grads = [[torch.from_numpy((rng.standard_normal(s) * 1e-2).astype(np.float32)).to(gd).float().numpy()
              for s in SHAPES] for _ in range(steps)]
    return init, grads


def _muon(params):
    return torch.optim.Muon([dict(params=params[:SPLIT], **GROUPS[0]), dict(params=params[SPLIT:], **GROUPS[1])])


def _make(variant, init, dev, dtype=torch.float32, **kw):
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dtype).to(dev)) for a in init]
    return params, module_for(variant).ShardedOptimizer(_muon(params), **kw)


def _step(opt, params, step, dev):
    opt.zero_grad()
    for p, g in zip(params, step):
        set_grad(p, torch.from_numpy(g.copy()).to(p.dtype).to(dev))
    opt.step()


def _bits(params):
    return [p.detach().cpu().contiguous().view(torch.int16).numpy().copy() for p in params]


def _master(opt, p):
    """The fp32 weights the update keeps: the parameter, or the split master of a bf16 one."""
    from zero_amd._update import join_split_master

    st = opt.optimizer.state[p]
    return (join_split_master(p, st["master_residual"]) if "master_residual" in st else p).detach().cpu().double().numpy()


@pytest.mark.parametrize("variant,dtype", [(1, torch.float32), (2, torch.float32), (2, torch.bfloat16)])
def test_trajectory_against_float64_oracle(gpu, pg1, variant, dtype):
    init, grads = _inputs(3, dtype)
    ref = [a.astype(np.float64) for a in init]
    rbuf = [np.zeros_like(a) for a in ref]
    cpu = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
    cpu_opt = _muon(cpu)
    params, opt = _make(variant, init, gpu, dtype)
    for t, step in enumerate(grads):
        _step(opt, params, step, gpu)
        for q, g in zip(cpu, step):
            q.grad = torch.from_numpy(g.copy())
        cpu_opt.step()
        for i, g in enumerate(step):
            ref[i], rbuf[i] = mo.step(ref[i], g.astype(np.float64), rbuf[i], **GROUPS[i >= SPLIT])
            ours = np.linalg.norm(_master(opt, params[i]) - ref[i])
            theirs = np.linalg.norm(cpu[i].detach().double().numpy() - ref[i])
            slack = float(np.spacing(np.float32(np.abs(ref[i]).max()))) * ref[i].size ** 0.5
            print(f"step {t} param {i}: ours {ours:.3e}, torch fp32 {theirs:.3e}")
            assert ours <= 1.5 * theirs + slack
            buf = opt.optimizer.state[params[i]]["momentum_buffer"]  # a live fp32 view, torch's bits
            assert buf.shape == params[i].shape and torch.equal(buf.cpu(), cpu_opt.state[cpu[i]]["momentum_buffer"])


def test_checkpoint_continues_bit_for_bit(gpu, pg1):
    init, grads = _inputs(4, torch.bfloat16)
    params, opt = _make(2, init, gpu, torch.bfloat16)
    for step in grads:
        _step(opt, params, step, gpu)
    pa, oa = _make(2, init, gpu, torch.bfloat16)
    for step in grads[:2]:
        _step(oa, pa, step, gpu)
    sd = oa.state_dict()
    assert set(sd["state"][0]) == {"momentum_buffer", "master_residual"}  # torch's entry + the master
    pb, ob = _make(2, [p.detach().float().cpu().numpy() for p in pa], gpu, torch.bfloat16)
    ob.load_state_dict(sd)
    for step in grads[2:]:
        _step(ob, pb, step, gpu)
    assert all(np.array_equal(_master(ob, p), _master(opt, q)) for p, q in zip(pb, params))


def test_a_second_optimizer_takes_the_rest_of_the_model(gpu, pg1):
    """Muon refuses non-2-D parameters: AdamW in a ShardedOptimizer of its own over the biases."""
    from zero_amd import zero2

    init, grads = _inputs(2)
    bias = [np.linspace(-1, 1, n).astype(np.float32) for n in (70, 40)]
    params, opt = _make(2, init, gpu)
    bs = [torch.nn.Parameter(torch.from_numpy(b.copy()).to(gpu)) for b in bias]
    opt_b = zero2.ShardedOptimizer(torch.optim.AdamW(bs, lr=1e-2))
    cpu = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init + bias]
    cpu_m, cpu_a = _muon(cpu[:len(init)]), torch.optim.AdamW(cpu[len(init):], lr=1e-2)
    for step in grads:
        opt_b.zero_grad()
        for b in bs:
            set_grad(b, torch.full_like(b, 0.25))
        _step(opt, params, step, gpu)
        opt_b.step()
        for q, g in zip(cpu, step + [np.full_like(b, 0.25) for b in bias]):
            q.grad = torch.from_numpy(g.copy())
        cpu_m.step()
        cpu_a.step()
    for p, q in zip(params + bs, cpu):
        assert torch.allclose(p.detach().cpu(), q.detach(), rtol=0, atol=2e-3 * float(q.detach().abs().max()))


def _ws_worker(rank, ws, port, want):
    """Identical gradients on every rank: the world-size-1 run's parameters, bit for bit."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    init_pg(rank, ws, port)
    init, grads = _inputs(2, short=True)
    params, opt = _make(2, init, dev, comm=test_comm(), bucket_mb=ws * 64 * 4 / (1 << 20))
    assert opt.engine.K > 1  # several rounds: a matrix's gradient arrives in pieces
    for t, step in enumerate(grads):
        _step(opt, params, step, dev)
        torch.cuda.synchronize()
        for i, (got, exp) in enumerate(zip(_bits(params), want[t])):
            assert np.array_equal(got, exp), (ws, rank, t, i)
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
            want.append(_bits(params))
    finally:
        dist.destroy_process_group()
    del opt, params
    spawn_batch(ws, [(_ws_worker, (want,))])


REFUSED = [(2, dict(layout="flat")), (2, dict(arena="buckets")), (2, dict(overlap=True)),
           (2, dict(grad_comm="bf16")), (2, dict(max_grad_norm=1.0)),
           (2, dict(max_grad_norm=1.0, skip_nonfinite=True)), (2, dict(max_grad_norm=1.0, param_grad_norms=True)),
           (2, dict(state_dtype=torch.bfloat16)), (2, dict(state_dtype=torch.bfloat16, state_rounding="stochastic")),
           (2, dict(master="none")), (2, dict(ema_decay=0.99)), (2, dict(param_update_norms=True)),
           (3, dict()), (3, dict(update=True)), (3, dict(update=True, grad_accumulation=True)), (1, "carry")]


@pytest.mark.parametrize("variant,kw", REFUSED)
def test_unsupported_combinations_are_refused_at_construction(gpu, pg1, variant, kw):
    from zero_amd._update import check_muon

    init, _ = _inputs(0)
    with pytest.raises(ValueError, match="Muon"):
        if kw == "carry":  # ZeRO-1 at world size > 1: what the constructor passes there
            check_muon(carry=True)
        else:
            _make(variant, init, gpu, **kw)
