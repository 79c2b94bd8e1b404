"""``ShardedOptimizer(ScheduleFreeAdamW(...))`` on ZeRO-1/2/3 in lockstep with the class itself on
fp32 CPU tensors, bit for bit; the split master of bf16 parameters (the parameter joined with its
residual) follows the class on the widened values.  ZeRO-1 at world size 2 (the carry) runs
against tests/_sfadam_oracle.py on gradients that differ per rank."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _sfadam_oracle as so
from _zero_run import init_pg, module_for, set_grad, spawn_batch
from test_gpu_lion_optimizer import _host, _same, _z3_set_grad, pg1  # noqa: F401  (pg1: a fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(64, 48), (48,), (33, 7), (1,)]
HP = dict(lr=2.5e-3, betas=(0.9, 0.99), weight_decay=0.1, warmup_steps=2)


def _make(variant, dev, dtype, scale, **kw):
    from zero_amd.optim import ScheduleFreeAdamW

    gen = torch.Generator().manual_seed(5)
    rnd = lambda s, k: (torch.randn(s, generator=gen) * k).to(dtype)  # noqa: E731
    init = [rnd(s, 0.05) for s in SHAPES]
    grads = [[rnd(s, 1e-2 * scale) for s in SHAPES] for _ in range(4)]
    ref = ScheduleFreeAdamW([torch.nn.Parameter(a.float().clone()) for a in init], **HP)
    opt = ScheduleFreeAdamW([torch.nn.Parameter(a.clone().to(dev)) for a in init], **HP)
    return grads, ref, module_for(variant).ShardedOptimizer(opt, **kw)


def _step(opt, ref, gs, variant):
    opt.zero_grad()
    for p, g in zip(opt.params, gs):
        (_z3_set_grad if variant == 3 else set_grad)(p, g.clone().to(p.device))
    opt.step()
    coef = 1.0 if opt.max_grad_norm is None else torch.tensor(float(opt.last_clip_coef))
    for q, g in zip(ref.param_groups[0]["params"], gs):
        q.grad = g.float() * coef  # (clipped: times the coefficient the step read)
    ref.step()
    return coef


def _check(opt, ref, variant, what):
    from zero_amd._update import join_split_master

    for i, (p, q) in enumerate(zip(opt.params, ref.param_groups[0]["params"])):
        if p.dtype == torch.float32:
            _same(_host(p), _host(q), f"{what} param {i}")
        if variant != 3 and i not in opt.local_param_indices:
            continue
        st = opt.optimizer.state[p]
        _same(_host(st["z"]), _host(ref.state[q]["z"]), f"{what} z {i}")
        _same(_host(st["exp_avg_sq"]), _host(ref.state[q]["exp_avg_sq"]), f"{what} exp_avg_sq {i}")
        if p.dtype != torch.float32:  # the split master: in place, so it is what the parameter shows
            lo = (opt._state_views(i) if variant == 3 else opt.engine.state_views(i))["master_residual"]
            _same(_host(join_split_master(p, lo)), _host(q), f"{what} split master {i}")


def _trajectory(variant, dev, dtype=torch.float32, what="", clip=None, reload=False, **kw):
    """4 steps with the eval() / train() pair after the second, compared after every call;
    ``clip``: max_grad_norm, its coefficient checked against clip_grad_norm_'s formula in double;
    ``reload``: instead of the pair, state_dict() into a fresh wrapper for the last two steps."""
    kw = dict(kw, **({"update": True} if variant == 3 else {}),
              **({} if clip is None else {"max_grad_norm": clip}))
    scale = 1.0 if clip is None else 3.0  # (a gradient norm of about 1.7)
    grads, ref, opt = _make(variant, dev, dtype, scale, **kw)
    for t, gs in enumerate(grads):
        coef = _step(opt, ref, gs, variant)
        _check(opt, ref, variant, f"{what} step {t}")
        assert opt.optimizer.param_groups[0]["k"] == ref.param_groups[0]["k"] == t + 1
        if clip is not None:
            norm = float(torch.cat([g.double().reshape(-1) for g in gs]).norm())
            assert norm > 1.0 and abs(float(coef) - clip / (norm + 1e-6)) <= 1e-6 * float(coef)
        if t == 1 and reload:
            sd, old = opt.state_dict(), opt
            assert sd["param_groups"][0]["k"] == 2 and sd["param_groups"][0]["train_mode"] is True
            opt = _make(variant, dev, dtype, scale, **kw)[2]
            with torch.no_grad():
                for c, b in zip(opt.params, old.params):
                    c.data.copy_(b.data)
            opt.load_state_dict(sd)
        elif t == 1:
            for name in ("eval", "train"):
                for o in (opt, opt, ref):  # (the wrapper twice: idempotent)
                    getattr(o, name)()
                _check(opt, ref, variant, f"{what} {name}")
                if name == "eval":
                    for call in (opt.step, opt.state_dict):
                        with pytest.raises(RuntimeError, match="eval mode"):
                            call()
    steps = [float(opt.optimizer.state[p]["step"]) for p in opt.params if "step" in opt.optimizer.state[p]]
    assert steps and set(steps) == {4.0}
    return opt


@pytest.mark.parametrize("variant,dtype", [(1, torch.float32), (2, torch.float32), (3, torch.float32),
                                           (2, torch.bfloat16), (3, torch.bfloat16)])
def test_ws1_equals_the_class_on_the_cpu(gpu, pg1, variant, dtype):  # noqa: F811
    opt = _trajectory(variant, gpu, dtype)
    core = opt._core if variant == 3 else opt.engine
    assert core.kind == "sfadam" and core.v is not None and core.vmax is None


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("kw", [dict(clip=0.5), dict(reload=True)], ids=["max_grad_norm", "checkpoint"])
def test_ws1_clipped_and_reloaded_equal_the_class(gpu, pg1, variant, kw):  # noqa: F811
    _trajectory(variant, gpu, **kw)


def _ws2_worker(rank, ws, port):
    """The same gradients on both ranks average to the gradient; 64-element windows: several rounds."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    opt = _trajectory(2, torch.device("cuda:0"), what=f"rank {rank}", comm=test_comm(),
                      bucket_mb=ws * 64 * 4 / (1 << 20))
    assert opt.engine.K > 1 and 0 < len(opt.local_param_indices) < len(SHAPES)
    dist.destroy_process_group()


def test_zero2_ws2_equals_ws1(gpu):
    spawn_batch(2, [(_ws2_worker, ())])


class _CarryRef:
    """ZeRO-1 at world size ``ws`` in numpy, over whole flat parameters: tests/_sfadam_oracle.py's
    element on the summed gradient with ``grad_div = ws`` and ``carry_mul = ws - 1``, the carry (the
    last averaged gradient, which ZeRO-1's surviving gradients hold) kept from step to step."""

    def __init__(self, init, ws):
        self.ws = ws
        self.y = [a.copy() for a in init]
        self.z = [a.copy() for a in init]  # starts as a copy of the parameter
        self.v = [np.zeros_like(a) for a in init]
        self.carry = [np.zeros_like(a) for a in init]
        self.sched = so.schedule(HP["lr"], 8, warmup_steps=HP["warmup_steps"])
        self.k = 0

    def step(self, sums):
        t, lr_t, c = self.sched[self.k]
        self.k += 1
        hp = so.SfHP(lr_t, *HP["betas"], 1e-8, HP["weight_decay"], t, c,
                     grad_div=float(self.ws), carry_mul=float(self.ws - 1))
        for i, g in enumerate(sums):
            self.y[i], self.z[i], self.v[i], self.carry[i] = so.sfadam_elem(
                g, self.y[i], self.z[i], self.v[i], hp, carry=self.carry[i])

    def swap(self, to_eval):
        self.y = [so.swap(y, z, HP["betas"][0], to_eval) for y, z in zip(self.y, self.z)]


def _z1_carry_worker(rank, ws, port):
    """ZeRO-1 keeps its carry through opt.zero_grad(): integer gradients that differ per rank (their
    sum is exact whatever the order), 3 steps with the eval() / train() pair after the second;
    64-element windows, so several rounds."""
    from _gloo_comm import test_comm
    from zero_amd.optim import ScheduleFreeAdamW

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    init = [(rng.standard_normal(int(np.prod(s))) * 0.05).astype(np.float32) for s in SHAPES]
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).reshape(s).to(dev))
              for a, s in zip(init, SHAPES)]
    opt = module_for(1).ShardedOptimizer(ScheduleFreeAdamW(params, **HP), comm=test_comm(),
                                         bucket_mb=ws * 64 * 4 / (1 << 20))
    eng = opt.engine
    assert eng.kind == "sfadam" and eng.K > 1 and eng.carry is not None
    assert 0 < len(opt.local_param_indices) < len(SHAPES)
    ref = _CarryRef(init, ws)

    def check(what):
        for i, p in enumerate(params):
            _same(_host(p), ref.y[i], f"rank {rank} {what} param {i}")
            if i not in opt.local_param_indices:
                continue
            st = opt.optimizer.state[p]
            _same(_host(st["z"]), ref.z[i], f"rank {rank} {what} z {i}")
            _same(_host(st["exp_avg_sq"]), ref.v[i], f"rank {rank} {what} exp_avg_sq {i}")
            off = int(eng.pieces.stream_off[eng.pieces.param == i][0])
            _same(_host(eng.carry[off:off + p.numel()]), ref.carry[i], f"rank {rank} {what} carry {i}")

    for t in range(3):
        local = [[rng.integers(-8, 9, a.size).astype(np.float32) for a in init] for _ in range(ws)]
        opt.zero_grad()
        for p, g, s in zip(params, local[rank], SHAPES):
            set_grad(p, torch.from_numpy(g.copy()).reshape(s).to(dev))
        opt.step()
        ref.step([np.sum(np.stack([local[r][i] for r in range(ws)]), axis=0, dtype=np.float32)
                  for i in range(len(init))])
        check(f"step {t}")
        if t >= 1:  # the carry is in the sum: the step on the summed gradient alone gives other bits
            assert any(np.any(c != 0) for c in ref.carry)
        if t == 1:
            for name in ("eval", "train"):
                getattr(opt, name)()
                ref.swap(name == "eval")
                check(name)
    assert opt.optimizer.param_groups[0]["k"] == 3
    dist.destroy_process_group()


def test_zero1_ws2_keeps_the_carry(gpu):
    """ZeRO-1 at world size 2, the CARRY instances behind the wrapper, against the numpy oracle."""
    spawn_batch(2, [(_z1_carry_worker, ())])
