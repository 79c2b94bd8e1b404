"""``ShardedOptimizer(zero_amd.optim.LAMB(...))`` against tests/_lamb_oracle.py: m and v bit for
bit, the trust ratios within (k + 4) * 2^-24 of the oracle's float64 ones (the bound and k:
tests/test_gpu_lamb_kernel.py), the master bit for bit when the oracle applies each step's
``last_trust_ratios``.  ZeRO-1/2 at world size 1; world sizes 2 and 3 (gloo-staged) on ZeRO-2's
``layout="flat"`` and ZeRO-3 update mode, which cut parameters across ranks.  The gradients are
multiples of 2^-8, so the ranks' sum is exact in any order.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _lamb_oracle as lo
from oracle import c_oracle
from _zero_run import init_pg, module_for, spawn_batch
from test_gpu_clip_optimizer import pg1  # noqa: F401
from test_gpu_zero3_accumulate import Probe, ProbeModel

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5), (2 * 4096 + 37,), (1,), (600,)]  # below a chunk, several chunks, one element
GROUPS = [([0, 1], dict(lr=2e-3, weight_decay=0.01)), ([2, 3], dict(lr=1e-3, weight_decay=0.0))]
BETAS, EPS = (0.9, 0.999), 1e-6


def _grad(step, rank, i):
    rng = np.random.default_rng(1000 * step + 10 * rank + i)
    return (rng.integers(-64, 65, int(np.prod(SHAPES[i]))) / 256.0).astype(np.float32)


def _build(engine, dev, dtype, init, **kw):
    from zero_amd import zero3
    from zero_amd.optim import LAMB

    model = ProbeModel([Probe(torch.from_numpy(w.copy()).to(dev, dtype).view(s))
                        for w, s in zip(init, SHAPES)])
    params = [m.weight for m in model.probes]
    inner = LAMB([dict(params=[params[i] for i in idx], **g) for idx, g in GROUPS], betas=BETAS,
                 eps=EPS)
    if engine != 3:
        return model, params, module_for(engine).ShardedOptimizer(inner, **kw)
    opt = zero3.ShardedOptimizer(inner, update=True, bucket_mb=0.02, **kw)
    zero3.register_zero3_hooks(model, opt.param_managers)
    return model, params, opt


def _backward(model, step, rank, live=None):
    for i, m in enumerate(model.probes):
        m.c = torch.from_numpy(_grad(step, rank, i)).to(m.weight.device, m.weight.dtype).view(SHAPES[i])
    model([live is None or i in live for i in range(len(SHAPES))]).backward()


def _shard(opt, name):
    """[(parameter, offset in it, fp32 values)] of this rank's pieces of m / v / the master."""
    from zero_amd._update import join_split_master

    if hasattr(opt, "_core"):  # ZeRO-3: the chunk arena
        ar, core, win = opt._arena, opt._core, opt._arena.P
        pcs = [(i, r[0] * r[2], int(s), int(n)) for i, (r, s, n) in enumerate(zip(ar.rows, ar.slot, ar.ln))]
    else:
        core, pc, win = opt.engine, opt.engine.pieces, opt.engine.own_window()
        pcs = zip(*(x.tolist() for x in (pc.param, pc.param_off, pc.stream_off, pc.length)))
    x = getattr(core, name) if name != "master" else core.master  # (master="fp32": in the shard)
    if x is None:  # the parameter arena itself, or its words joined with the residuals
        x = win if core.lo is None else join_split_master(win[:len(core.lo)], core.lo)
    return [(i, po, x[so:so + n].float().cpu().numpy()) for i, po, so, n in pcs]


def _run(engine, dev, dtype, rank=0, ws=1, steps=3, skip=None, **kw):
    from zero_amd.kernels import adam_groups

    k = 4 * adam_groups(dtype == torch.bfloat16 and kw.get("master") != "fp32")
    rng = np.random.default_rng(3)
    P = [torch.from_numpy(rng.standard_normal(int(np.prod(s))).astype(np.float32)).to(dtype)
         .float().numpy() for s in SHAPES]
    model, params, opt = _build(engine, dev, dtype, P, **kw)
    M, V = [np.zeros_like(w) for w in P], [np.zeros_like(w) for w in P]
    count = [0] * len(P)
    for step in range(steps):
        live = [i for i in range(len(P)) if (step, i) != skip]
        if engine != 3:
            opt.zero_grad()
        _backward(model, step, rank, live)
        opt.step()
        ratios = opt.last_trust_ratios.cpu().numpy()
        coef = np.float32(float(opt.last_clip_coef)) if "max_grad_norm" in kw else None
        for i in live:
            g = sum(_grad(step, r, i) for r in range(ws))  # (exact: multiples of 2^-8)
            count[i] += 1
            gi = next(j for j, (idx, _) in enumerate(GROUPS) if i in idx)
            hp = lo.LambHP(GROUPS[gi][1]["lr"], *BETAS, EPS, GROUPS[gi][1]["weight_decay"],
                           count[i], grad_div=float(ws))
            *_, (_, _, r64, _) = lo.step(P[i], g, M[i], V[i], hp, coef=coef, norms64=True)
            assert abs(float(ratios[i]) - r64) <= (k + 4) * 2.0 ** -24 * r64
            P[i], M[i], V[i], _, _ = lo.step(P[i], g, M[i], V[i], hp, coef=coef,
                                             neg_s=-(hp.lr * np.float32(ratios[i])))
            if k == 16:  # as the split master stores it: an exact tie's residual moves it 1 ulp
                P[i] = c_oracle.join_master(*c_oracle.split_master(P[i]))
        assert skip is None or skip[0] != step or ratios[skip[1]] == 1.0
        for name, ref in (("m", M), ("v", V), ("master", P)):
            for i, po, x in _shard(opt, name):
                assert np.array_equal(x.view(np.uint32), ref[i][po:po + len(x)].view(np.uint32)), \
                    (name, step, i)
    return model, params, opt


@pytest.mark.parametrize("engine", [1, 2])
@pytest.mark.parametrize("dtype,master", [(torch.float32, "split"), (torch.bfloat16, "split"),
                                          (torch.bfloat16, "fp32")])
def test_ws1_three_steps(gpu, pg1, engine, dtype, master):
    _, _, opt = _run(engine, gpu, dtype, master=master, skip=(1, 3))
    un, wn = opt.last_param_update_norms, opt.last_param_weight_norms
    assert un.shape == wn.shape == (len(SHAPES),) and bool((un > 0).all())


def test_ws1_clipped(gpu, pg1):
    """The moments see the clipped gradient; the oracle takes the engine's own coefficient."""
    _, _, opt = _run(2, gpu, torch.bfloat16, steps=2, max_grad_norm=0.5)
    assert 0 < float(opt.last_clip_coef) < 1


def test_checkpoint_round_trip(gpu, pg1):
    model, params, opt = _run(2, gpu, torch.bfloat16, steps=2)
    sd = opt.state_dict()
    assert {"exp_avg", "exp_avg_sq", "step"} <= set(sd["state"][0])
    model2, params2, opt2 = _build(2, gpu, torch.bfloat16,
                                   [p.detach().float().cpu().numpy().reshape(-1) for p in params])
    opt2.load_state_dict(sd)
    for m, o in ((model, opt), (model2, opt2)):
        o.zero_grad()
        _backward(m, 2, 0)
        o.step()
    torch.cuda.synchronize()
    for a, b in zip(params, params2):
        assert torch.equal(a.detach().view(torch.int16), b.detach().view(torch.int16))
    assert torch.equal(opt.last_trust_ratios, opt2.last_trust_ratios)


def test_refusals(gpu, pg1):
    from zero_amd import zero2, zero3
    from zero_amd._update import check_lamb
    from zero_amd.optim import LAMB

    mk = lambda dt=torch.float32: LAMB([torch.nn.Parameter(torch.zeros(8, device=gpu, dtype=dt))])  # noqa: E731
    for kw in (dict(arena="buckets"), dict(overlap=True), dict(ema_decay=0.9),
               dict(max_grad_norm=1.0, skip_nonfinite=True), dict(state_dtype=torch.bfloat16),
               dict(param_update_norms=True)):
        with pytest.raises(ValueError, match="LAMB"):
            zero2.ShardedOptimizer(mk(), **kw)
    with pytest.raises(ValueError, match="LAMB"):
        zero2.ShardedOptimizer(mk(torch.bfloat16), master="none")
    with pytest.raises(ValueError, match="LAMB.*ZeRO-1 at world size > 1"):
        check_lamb(carry=True)
    with pytest.raises(ValueError, match="LAMB.*ZeRO-3 reference mode"):
        zero3.ShardedOptimizer(mk(), update=False)


def _worker(rank, ws, port, engine, steps, kw):
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    _run(engine, torch.device("cuda:0"), torch.float32, rank=rank, ws=ws, steps=steps,
         comm=test_comm(), **kw)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_parameters_cut_across_ranks(gpu, ws):
    spawn_batch(ws, [(_worker, (2, 3, dict(layout="flat")))] +
                [(_worker, (3, 2, {}))] * (ws == 2))
