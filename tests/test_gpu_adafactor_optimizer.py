"""torch.optim.Adafactor behind the ZeRO-1/2 ShardedOptimizer: the trajectory against torch's own
float64 run, world sizes 2 and 3 against world size 1 bit for bit, a parameter without a gradient,
and checkpoints."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from _zero_run import init_pg, module_for, set_grad, spawn_batch
from conftest import free_port

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (24,), (2, 9, 16), (70, 8), (5,), (1, 40)]
SPLIT = 3  # parameters [0, SPLIT) are group 0
EPS1 = 2.0 ** -23
GROUPS = [dict(lr=1e-2, weight_decay=0.1), dict(lr=3e-3, weight_decay=0.0, d=2.0, beta2_decay=-0.7)]


@pytest.fixture
def pg1():
    init_pg(0, 1, free_port())
    yield
    dist.destroy_process_group()


def _inputs(steps, seed=3, scale=1e-2, short=False):
    """``short``: gradients with 8 significant bits, so that the sum over 2 or 3 ranks and its
    division by the world size are exact (fp32 (g + g + g) / 3 is not g in general)."""
    rng = np.random.default_rng(seed)
    init = [(rng.standard_normal(s) * 0.05).astype(np.float32) for s in SHAPES]
    grads = [[(rng.standard_normal(s) * scale).astype(np.float32) for s in SHAPES] for _ in range(steps)]
    if short:
        grads = [[torch.from_numpy(g).bfloat16().float().numpy() for g in step] for step in grads]
    return init, grads


def _adafactor(params):
    return torch.optim.Adafactor([dict(params=params[:SPLIT], **GROUPS[0]),
                                  dict(params=params[SPLIT:], **GROUPS[1])], eps=(EPS1, 1e-3),
                                 foreach=False)


def _torch_run(init, grads, dtype):
    """torch's own CPU Adafactor in ``dtype``: parameters and state after the last step."""
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dtype)) for a in init]
    opt = _adafactor(ps)
    for step in grads:
        for p, g in zip(ps, step):
            p.grad = None if g is None else torch.from_numpy(g.copy()).to(dtype)
        opt.step()
    return ps, opt


def _make(variant, init, dev, **kw):
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in init]
    return params, module_for(variant).ShardedOptimizer(_adafactor(params), **kw)


def _step(opt, params, step, dev):
    opt.zero_grad()
    for p, g in zip(params, step):
        if g is not None:
            set_grad(p, torch.from_numpy(g.copy()).to(dev))
    opt.step()


def _bits(params):
    return [p.detach().cpu().numpy().view(np.uint32).copy() for p in params]


def _normwise(a, b):
    a, b = a.detach().cpu().double().numpy(), b.detach().double().numpy()
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize("variant", [1, 2])
def test_trajectory_against_torch_float64(gpu, pg1, variant):
    init, grads = _inputs(3)
    ref, ref_opt = _torch_run(init, grads, torch.float64)
    f32, f32_opt = _torch_run(init, grads, torch.float32)
    params, opt = _make(variant, init, gpu)
    for step in grads:
        _step(opt, params, step, gpu)
    for i, (p, q, r) in enumerate(zip(params, ref, f32)):
        st, rst, fst = opt.optimizer.state[p], ref_opt.state[q], f32_opt.state[r]
        names = ("row_var", "col_var") if p.dim() > 1 else ("variance",)
        assert set(names) <= set(st) and float(st["step"]) == 3
        pairs = [(p, q, r)] + [(st[k], rst[k], fst[k]) for k in names]
        for got, want, torch32 in pairs:
            own, theirs = _normwise(got, want), _normwise(torch32, want)
            print(f"param {i}: ours {own:.2e}, torch fp32 {theirs:.2e}")
            assert theirs < 5e-6 and own <= 5e-6  # (the bound stands on torch's own fp32 deviation)


def test_a_parameter_without_gradient_keeps_value_state_and_step(gpu, pg1):
    init, grads = _inputs(2)
    params, opt = _make(2, init, gpu)
    _step(opt, params, grads[0], gpu)
    before = (_bits(params)[3], {k: v.clone() for k, v in opt.optimizer.state[params[3]].items()})
    step = list(grads[1])
    step[3] = None
    _step(opt, params, step, gpu)
    st = opt.optimizer.state[params[3]]
    assert np.array_equal(_bits(params)[3], before[0])
    assert float(st["step"]) == 1 and float(opt.optimizer.state[params[0]]["step"]) == 2
    for k in ("row_var", "col_var"):
        assert torch.equal(st[k], before[1][k])


def test_checkpoint_continues_bit_for_bit_and_a_torch_state_dict_loads(gpu, pg1):
    init, grads = _inputs(4)
    params, opt = _make(2, init, gpu)
    for step in grads:
        _step(opt, params, step, gpu)
    want = _bits(params)
    pa, oa = _make(2, init, gpu)
    for step in grads[:2]:
        _step(oa, pa, step, gpu)
    sd = oa.state_dict()
    pb, ob = _make(2, [p.detach().cpu().numpy() for p in pa], gpu)
    ob.load_state_dict(sd)
    for step in grads[2:]:
        _step(ob, pb, step, gpu)
    assert all(np.array_equal(a, b) for a, b in zip(_bits(pb), want))
    # a plain unsharded torch.optim.Adafactor.state_dict() loads by index
    cpu, cpu_opt = _torch_run(init, grads[:1], torch.float32)
    pc, oc = _make(2, init, gpu)
    oc.load_state_dict(cpu_opt.state_dict())
    for p, q in zip(pc, cpu):
        st, want_st = oc.optimizer.state[p], cpu_opt.state[q]
        assert float(st["step"]) == 1
        for k in (("row_var", "col_var") if p.dim() > 1 else ("variance",)):
            assert torch.equal(st[k].cpu(), want_st[k])


def _ws_worker(rank, ws, port, want):
    """Identical gradients on every rank: every parameter after each step equals the world-size-1
    run's bit for bit (ownership independence, and the broadcast)."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    init, grads = _inputs(2, short=True)
    params, opt = _make(2, init, dev, comm=test_comm(), bucket_mb=ws * 64 * 4 / (1 << 20))
    assert opt.engine.K > 1  # several rounds: a parameter's gradient arrives in pieces
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
