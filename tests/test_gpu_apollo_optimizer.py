"""zero_amd.optim.Apollo behind the ZeRO-1/2 ShardedOptimizer, in the form of the Adam-mini optimizer
test: the trajectory over 4 steps with update_proj_gap=2 against the float64 oracle with the class's
own fp32 CPU step as the yardstick (the fused run may lie 1.5 times as far from float64), world
sizes 2 and 3 against world size 1 bit for bit (every state entry), a checkpoint across the re-draw
at step 3, and the refusals."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _apollo_oracle as ao
from _zero_run import init_pg, module_for, spawn_batch
from conftest import free_port
from test_gpu_muon_optimizer import _bits, _step, pg1  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 24), (70, 8), (9, 144)]
SPLIT = 2  # parameters [0, SPLIT) are group 0
GROUPS = [dict(lr=1e-2, weight_decay=0.1, rank=16),
          dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, rank=1, scale=128.0, scale_type="tensor", seed=9)]
KW = [dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, rank=16, scale=1.0,
           scale_type="channel", seed=0),
      dict(lr=3e-3, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.0, rank=1, scale=128.0,
           scale_type="tensor", seed=9)]
STATE = ("exp_avg", "exp_avg_sq", "scaled_grad_norm", "seed")


def _inputs(steps, dtype=torch.float32, short=False):
    rng = np.random.default_rng(3)
    rnd = lambda a, dt: torch.from_numpy(a.astype(np.float32)).to(dt).float().numpy()  # noqa: E731
    init = [rnd(rng.standard_normal(s) * 0.05, dtype) for s in SHAPES]
    grads = [[rnd(rng.standard_normal(s) * 1e-2, dtype) for s in SHAPES] for _ in range(steps)]
    if short:
        # 6 significant bits: the sketch reads bf16(sum over ranks), and 3 g then still fits bf16's 8,
        # as the sum / ws is exact.  The scale fp32(1 / (ws sqrt(rank))) is off 1 / (3 sqrt(rank)) by
        # 2^-25 relative at these ranks (1 and 16: a third of an ulp of 1.0101..b), less than half an
        # ulp of any product, so S, and everything after it, has the bits of world size 1.
        grads = [[(g.view(np.int32) & ~np.int32((1 << 18) - 1)).view(np.float32) for g in step] for step in grads]
    return init, grads


def _apollo(params):
    from zero_amd.optim import Apollo

    return Apollo([dict(params=params[:SPLIT], **GROUPS[0]), dict(params=params[SPLIT:], **GROUPS[1])],
                  update_proj_gap=2)


def _make(variant, init, dev, dtype=torch.float32, **kw):
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dtype).to(dev)) for a in init]
    return params, module_for(variant).ShardedOptimizer(_apollo(params), **kw)


def _master(opt, p):
    from zero_amd._update import join_split_master

    st = opt.optimizer.state[p]
    w = st["master_param"] if "master_param" in st else \
        join_split_master(p, st["master_residual"]) if "master_residual" in st else p
    return w.detach().cpu().double().numpy()


def _state(opt, params):
    """The APOLLO state this rank holds (its owned parameters), as bits."""
    return {i: [opt.optimizer.state[p][k].cpu().numpy().reshape(-1).view(np.uint8) for k in STATE]
            for i, p in enumerate(params) if "exp_avg" in opt.optimizer.state[p]}


@pytest.mark.parametrize("variant,dtype,master", [(1, torch.float32, "split"), (2, torch.float32, "split"),
                                                  (2, torch.bfloat16, "split"), (2, torch.bfloat16, "fp32")])
def test_trajectory_against_float64_oracle(gpu, pg1, variant, dtype, master):  # noqa: F811
    init, grads = _inputs(4, dtype)
    ref = [a.astype(np.float64) for a in init]
    rm = [np.zeros((max(s), KW[i >= SPLIT]["rank"])) for i, s in enumerate(SHAPES)]
    rv, rf = [np.zeros_like(m) for m in rm], [0.0] * len(SHAPES)
    cpu = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
    cpu_opt = _apollo(cpu)
    params, opt = _make(variant, init, gpu, dtype, master=master)
    for t, step in enumerate(grads):
        _step(opt, params, step, gpu)
        for q, g in zip(cpu, step):
            q.grad = torch.from_numpy(g.copy())
        cpu_opt.step()
        for i, g in enumerate(step):
            kw = dict(KW[i >= SPLIT])
            ref[i], rm[i], rv[i], rf[i] = ao.step(ref[i], g.astype(np.float64), rm[i], rv[i], rf[i], t + 1,
                                                  update_proj_gap=2, norm_growth=1.01,
                                                  **{**kw, "seed": kw["seed"] + i})
            ours = np.linalg.norm(_master(opt, params[i]) - ref[i])
            theirs = np.linalg.norm(cpu[i].detach().double().numpy() - ref[i])
            print(f"step {t} param {i}: ours {ours:.3e}, class fp32 {theirs:.3e}, ratio {ours / theirs:.3f}")
            assert ours <= 1.5 * theirs
            st = opt.optimizer.state[params[i]]
            assert float(st["step"]) == t + 1 and int(st["seed"]) == kw["seed"] + i
            assert st["exp_avg"].shape == st["exp_avg_sq"].shape == rm[i].shape
            assert float(st["scaled_grad_norm"]) > 0 and bool((st["exp_avg_sq"] > 0).all())


def test_checkpoint_continues_bit_for_bit(gpu, pg1):  # noqa: F811
    init, grads = _inputs(4, torch.bfloat16)
    params, opt = _make(2, init, gpu, torch.bfloat16)
    for step in grads:
        _step(opt, params, step, gpu)
    pa, oa = _make(2, init, gpu, torch.bfloat16)
    for step in grads[:2]:
        _step(oa, pa, step, gpu)
    sd = oa.state_dict()
    assert set(sd["state"][0]) == {"step", *STATE, "master_residual"}
    pb, ob = _make(2, [p.detach().float().cpu().numpy() for p in pa], gpu, torch.bfloat16)
    ob.load_state_dict(sd)
    for step in grads[2:]:  # (step 3 re-draws sigma)
        _step(ob, pb, step, gpu)
    assert all(np.array_equal(_master(ob, p), _master(opt, q)) for p, q in zip(pb, params))
    assert all(np.array_equal(x, y) for a, b in zip(_state(ob, pb).values(), _state(opt, params).values())
               for x, y in zip(a, b))


def _ws_worker(rank, ws, port, want):
    """Identical gradients on every rank: the world-size-1 run's parameters and state, bit for bit."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    init_pg(rank, ws, port)
    init, grads = _inputs(3, short=True)
    with pytest.raises(ValueError, match=r"zero_amd\.optim\.Apollo is not supported with ZeRO-1 at world size > 1"):
        _make(1, init, dev, comm=test_comm())  # (on every rank, before anything collective)
    params, opt = _make(2, init, dev, comm=test_comm(), bucket_mb=ws * 64 * 4 / (1 << 20))
    for t, step in enumerate(grads):
        _step(opt, params, step, dev)
        torch.cuda.synchronize()
        for i, (got, exp) in enumerate(zip(_bits(params), want[t][0])):
            assert np.array_equal(got, exp), (ws, rank, t, i)
        state = _state(opt, params)
        assert sorted(state) == sorted(int(i) for i in opt.engine.owned_param_indices())
        assert all(np.array_equal(x, y) for i, v in state.items() for x, y in zip(v, want[t][1][i])), (ws, rank, t)
    dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_world_sizes_match_world_size_one(gpu, ws):
    init, grads = _inputs(3, short=True)
    init_pg(0, 1, free_port())
    try:
        params, opt = _make(2, init, gpu)
        want = []
        for step in grads:
            _step(opt, params, step, gpu)
            want.append((_bits(params), _state(opt, params)))
    finally:
        dist.destroy_process_group()
    del opt, params
    spawn_batch(ws, [(_ws_worker, (want,))])


@pytest.mark.parametrize("variant,kw,word", [
    (2, dict(layout="flat"), "layout"), (2, dict(arena="buckets"), "arena"), (2, dict(overlap=True), "overlap"),
    (2, dict(grad_comm="bf16"), "grad_comm"), (2, dict(max_grad_norm=1.0), "max_grad_norm"),
    (2, dict(skip_nonfinite=True), "skip_nonfinite"), (2, dict(param_grad_norms=True), "param_grad_norms"),
    (2, dict(state_dtype=torch.bfloat16), "state_dtype"),
    (2, dict(state_rounding="nearest"), "state_rounding"), (2, dict(master="none"), "master"),
    (2, dict(ema_decay=0.99), "ema_decay"), (2, dict(param_update_norms=True), "param_update_norms"),
    (3, {}, "ZeRO-3")])
def test_refusals_name_apollo_before_any_collective(gpu, pg1, variant, kw, word):  # noqa: F811
    init, _ = _inputs(0, torch.bfloat16)
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(torch.bfloat16).to(gpu)) for a in init]
    with pytest.raises(ValueError, match=rf"zero_amd\.optim\.Apollo is not supported with .*{word}"):
        module_for(variant).ShardedOptimizer(_apollo(params), **kw)
