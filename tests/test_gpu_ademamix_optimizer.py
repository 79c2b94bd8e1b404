"""``ShardedOptimizer(AdEMAMix(...))`` on ZeRO-1/2/3 in lockstep with the class on fp32 CPU tensors,
3 steps with both warm-ups over T = 2 (the cap is crossed), states and master bit for bit; a reloaded
checkpoint, a clipped run; world size 2 through the one-GPU communicator (ZeRO-1: with its carry)."""
import pytest
import torch
import torch.distributed as dist

from _zero_run import init_pg, module_for, set_grad, spawn_batch
from test_gpu_lion_optimizer import _chunk_of, _host, _same, _z3_set_grad, pg1  # noqa: F401  (pg1: a fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(70, 60), (48,), (33, 7)]  # 4,200 elements: past a chunk of either geometry
HP = dict(lr=1e-2, betas=(0.9, 0.99, 0.999), alpha=4.0, weight_decay=0.1, alpha_warmup=2, beta3_warmup=2)
NAMES = ("exp_avg", "exp_avg_slow", "exp_avg_sq")


def _make(variant, dev, dtype, scale, **kw):
    from zero_amd.optim import AdEMAMix

    gen = torch.Generator().manual_seed(5)
    rnd = lambda s, k: (torch.randn(s, generator=gen) * k).to(dtype)  # noqa: E731
    init = [rnd(s, 0.05) for s in SHAPES]
    grads = [[rnd(s, 1e-2 * scale) for s in SHAPES] for _ in range(3)]
    ref = AdEMAMix([torch.nn.Parameter(a.float().clone()) for a in init], **HP)
    opt = AdEMAMix([torch.nn.Parameter(a.clone().to(dev)) for a in init], **HP)
    return grads, ref, module_for(variant).ShardedOptimizer(opt, **kw)


def _check(opt, ref, variant, what, ws=1, rank=0):
    from zero_amd._update import join_split_master

    for i, (p, q) in enumerate(zip(opt.params, ref.param_groups[0]["params"])):
        cut = (lambda a: _chunk_of(_host(a), SHAPES[i], ws, rank)) if variant == 3 else _host
        if p.dtype == torch.float32:
            _same(_host(p), cut(q), f"{what} param {i}")
        if (variant != 3 and i not in opt.local_param_indices) or p.numel() == 0:
            continue
        st = opt.optimizer.state[p]
        assert float(st["step"]) == float(ref.state[q]["step"]) and "max_exp_avg_sq" not in st
        for name in NAMES:
            _same(_host(st[name]), cut(ref.state[q][name]), f"{what} {name} {i}")
        if p.dtype != torch.float32:  # the fp32 master of a bf16 parameter, joined or stored
            views = opt._state_views(i) if variant == 3 else opt.engine.state_views(i)
            mst = views["master_param"] if "master_param" in views else \
                join_split_master(p, views["master_residual"])
            _same(_host(mst), cut(q), f"{what} master {i}")


def _trajectory(variant, dev, dtype=torch.float32, what="", clip=None, reload=False, ws=1, rank=0, **kw):
    """3 steps, compared after each; ``reload``: after the second, state_dict() into a fresh wrapper.
    Every rank sets the same gradients; ZeRO-1 at ws > 1 adds ws - 1 times its carry (the last
    averaged gradient, which the surviving gradients hold) to the sum, and so does the class's feed."""
    carry = [0.0] * len(SHAPES) if variant == 1 and ws > 1 else None
    kw = dict(kw, **({"update": True} if variant == 3 else {}),
              **({} if clip is None else {"max_grad_norm": clip}))
    scale = 1.0 if clip is None else 3.0  # (a gradient norm of about 2)
    grads, ref, opt = _make(variant, dev, dtype, scale, **kw)
    for t, gs in enumerate(grads):
        opt.zero_grad()
        for p, g in zip(opt.params, gs):
            (_z3_set_grad if variant == 3 else set_grad)(p, g.clone().to(dev))
        opt.step()
        coef = 1.0 if clip is None else torch.tensor(float(opt.last_clip_coef))
        assert clip is None or float(coef) < 1.0
        for i, (q, g) in enumerate(zip(ref.param_groups[0]["params"], gs)):
            q.grad = g.float() * coef  # (clipped: times the coefficient the step read)
            if carry is not None:
                q.grad = carry[i] = (g.float() * ws + carry[i] * (ws - 1)) / ws
        ref.step()
        _check(opt, ref, variant, f"{what} step {t}", ws, rank)
        if t == 1 and reload:
            sd, old = opt.state_dict(), opt
            opt = _make(variant, dev, dtype, scale, **kw)[2]
            with torch.no_grad():
                for c, b in zip(opt.params, old.params):
                    c.data.copy_(b.data)
            opt.load_state_dict(sd)
    return opt


@pytest.mark.parametrize("variant,dtype,kw", [
    (1, torch.float32, {}), (2, torch.float32, {}), (3, torch.float32, {}), (1, torch.bfloat16, {}),
    (2, torch.bfloat16, dict(master="fp32")), (3, torch.bfloat16, {}), (2, torch.float32, dict(clip=0.5)),
    (2, torch.bfloat16, dict(reload=True)), (3, torch.float32, dict(reload=True))])
def test_ws1_equals_the_class_on_the_cpu(gpu, pg1, variant, dtype, kw):  # noqa: F811
    opt = _trajectory(variant, gpu, dtype, **kw)
    assert (opt._core if variant == 3 else opt.engine).kind == "ademamix"


def _ws2_worker(rank, ws, port, variant):
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    kw = dict(comm=test_comm(), **({} if variant == 3 else {"bucket_mb": ws * 64 * 4 / (1 << 20)}))
    opt = _trajectory(variant, torch.device("cuda:0"), what=f"z{variant} rank {rank}", ws=ws, rank=rank, **kw)
    if variant != 3:
        assert opt.engine.K > 1 and (opt.engine.carry is not None) == (variant == 1)  # several rounds
    dist.destroy_process_group()


def test_ws2_zero1_zero2_zero3(gpu):
    spawn_batch(2, [(_ws2_worker, (v,)) for v in (1, 2, 3)])
