"""``ShardedOptimizer(..., state_dtype=torch.bfloat16, state_rounding="stochastic")`` behind
ZeRO-2 and ZeRO-3: every optimizer wraps a stock ``torch.optim.Adam(params, lr=...)`` — torch's
default betas (0.9, 0.999), which bf16 moments rounded to nearest refuse.

Every trajectory is compared bit for bit with the restatement of tests/_bf16_state_sr_oracle.py
(widen the stored moments, the unchanged C oracle step, store them with the generator's bits for
(seed, the parameter's step, the element's index in its shard)); the indices come from the
optimizer's own layout.  World size 2 runs through real RCCL in one batch; ZeRO-3 also as rank 0 of
a simulated two-rank job, where the second step of a kind takes the cached sets.
"""
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist

import _accum32_oracle as a32
import _bf16_state_sr_oracle as so
import test_gpu_bf16_state_optimizer as bt
import test_gpu_zero3_accumulate_fp32 as z3t
from _zero_run import init_pg, set_grad, spawn_batch
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_clip_optimizer import pg1, rccl_env  # noqa: F401
from test_gpu_zero3_accumulate import Probe, ProbeModel, _rows

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999)  # torch.optim.Adam's defaults
SR = dict(state_dtype=BF16, state_rounding="stochastic")
SEED = (0xABCDEF << 32) | 0x13579B
host, _same = bt.host, bt._same


class _Ref(bt._Ref):
    """One parameter under the stochastic restatement; ``e``: its elements' shard indices."""

    def __init__(self, init, seed=SEED):
        super().__init__(init)
        self.seed, self.e = seed, None

    def step(self, g, div=1.0, coef=None, **hp):
        self.t += 1
        g = np.ascontiguousarray(g).reshape(-1)
        e, keys = np.asarray(self.e, np.uint64), so.keys_of(self.seed, self.t)
        if coef is not None:  # the unchanged fp32 step on the pre-clipped gradient
            gf = zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g
            with np.errstate(all="ignore"):
                gp = np.ascontiguousarray((gf / np.float32(div)).astype(np.float32) * np.float32(coef))
            chp = c_oracle.hparams(step=self.t, grad_div=1.0, **{**HP, **hp})
            p = c_oracle.join_master(self.hi, self.lo) if self.split else self.p
            so.adam_f32(p, gp, self.m, self.v, chp, e, keys)
            if self.split:
                self.hi, self.lo = c_oracle.split_master(p)
            return
        chp = c_oracle.hparams(step=self.t, grad_div=float(div), **{**HP, **hp})
        if self.split and g.dtype == np.uint16:
            so.adam_bf16_split(self.hi, self.lo, g, self.m, self.v, chp, e, keys)
        elif self.split:
            so.adam_f32grad_split(self.hi, self.lo, g, self.m, self.v, chp, e, keys)
        elif g.dtype == np.uint16:  # fp32 parameters, bf16 exchange
            so.adam_bf16(self.p, np.zeros(g.size, np.uint16), g, self.m, self.v, chp, e, keys)
        else:
            so.adam_f32(self.p, g, self.m, self.v, chp, e, keys)


def _offsets2(opt):
    """param index -> offset of its state in its owner's shard, from the engine's plan; the owned
    ones are checked against where their exp_avg view lies in the shard's m array."""
    eng, off = opt.engine, {}
    for r in range(opt.world_size):
        pc = eng.plan.pieces(r)
        for i, po, s, n in zip(pc.param.tolist(), pc.param_off.tolist(), pc.stream_off.tolist(),
                               pc.length.tolist()):
            if n > 0:
                assert po == 0 and n == opt.params[i].numel()
                off[i] = s
    for i in opt.local_param_indices:
        st = opt.optimizer.state[opt.params[i]]
        assert (st["exp_avg"].data_ptr() - eng.m.data_ptr()) // 2 == off[i]
    return off


def _bind2(opt, ref):
    off = _offsets2(opt)
    for i, r in enumerate(ref):
        r.e = off[i] + np.arange(opt.params[i].numel(), dtype=np.uint64)


# ---------------------------------------------------------------------------------------------
# world size 1: ZeRO-2 through a real backward
# ---------------------------------------------------------------------------------------------
def _mlp(gpu, dt):
    """Three small layers' worth of parameters: 96 x 97 = two chunks of 4,096 and a partial one,
    97 = 96 + a one-element scalar tail, 97 x 7 = 676 + a three-element one."""
    torch.manual_seed(0)
    mk = lambda *s: torch.nn.Parameter((torch.randn(*s) * 0.1).to(dt).to(gpu))  # noqa: E731
    w1, b1, w2 = mk(96, 97), mk(97), mk(97, 7)
    x, y = torch.randn(32, 96).to(dt).to(gpu), torch.randn(32, 7).to(dt).to(gpu)
    loss = lambda: (((torch.tanh(x @ w1 + b1) @ w2) - y) ** 2).sum()  # noqa: E731
    return [w1, b1, w2], loss


def _sq(grads):
    return sum(float(np.sum((zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g).astype(np.float64) ** 2))
               for g in grads)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16_split", "fp32"])
def test_ws1_zero2_through_backward(gpu, pg1, dt, clip):
    from zero_amd import zero2

    params, loss = _mlp(gpu, dt)
    ref = [_Ref(bt._init_of(p)) for p in params]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), state_seed=SEED,
                                 max_grad_norm=1.0 if clip else None, **SR)
    assert opt.state_rounding == opt.engine.state_rounding == "stochastic"
    assert opt.state_seed == opt.engine.state_seed == SEED
    assert opt.optimizer.param_groups[0]["betas"] == (0.9, 0.999)
    L = opt.engine.L
    assert opt.engine.state.numel() == bt._words(L, opt.engine.split)[0]  # the nearest layout
    _bind2(opt, ref)
    for t in range(1, 5):
        opt.zero_grad()
        (loss() * (1.0, 40.0, 0.05, 1.0)[t - 1]).backward()
        grads = [bt._grad_bits(p) for p in params]
        coef = None
        if clip and t == 1:
            opt.max_grad_norm = 4.0 * np.sqrt(_sq(grads))  # coefficients: 1, about 0.1, 1, 1
        opt.step()
        if clip:
            coef = np.float32(opt.last_clip_coef.item())
            assert (coef == 1.0) == (t != 2) and (t != 2 or 0.05 < coef < 0.2)
        assert opt.engine.last_adam_bytes == (18 if dt == BF16 else 20) * sum(p.numel() for p in params)
        for i, (p, r, g) in enumerate(zip(params, ref, grads)):
            r.step(g, coef=coef)
            r.check(p, opt.optimizer.state[p], f"step {t} param {i}")
            assert int(opt.optimizer.state[p]["step"].item()) == t


def test_ws1_fp32_master(gpu, pg1):
    from zero_amd import zero2

    params, loss = _mlp(gpu, BF16)
    init = [zo.bf16_bits_to_f32(host(p)) for p in params]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), master="fp32", state_seed=3, **SR)
    off = _offsets2(opt)
    m, v = [np.zeros(a.size, np.uint16) for a in init], [np.zeros(a.size, np.uint16) for a in init]
    for t in range(1, 5):
        opt.zero_grad()
        loss().backward()
        grads = [host(p.grad) for p in params]
        opt.step()
        assert opt.engine.last_adam_bytes == 20 * sum(p.numel() for p in params)
        for i, p in enumerate(params):
            pb = np.zeros(init[i].size, np.uint16)
            e = off[i] + np.arange(init[i].size, dtype=np.uint64)
            so.adam_bf16(init[i], pb, grads[i], m[i], v[i], c_oracle.hparams(step=t, **HP), e,
                         so.keys_of(3, t))
            st = opt.optimizer.state[p]
            _same(host(p), pb, f"step {t} param {i}")
            _same(host(st["master_param"]), init[i], f"step {t} master {i}")
            _same(host(st["exp_avg"]), m[i], f"step {t} exp_avg {i}")
            _same(host(st["exp_avg_sq"]), v[i], f"step {t} exp_avg_sq {i}")


# ---------------------------------------------------------------------------------------------
# injected gradients: step counts per parameter, checkpoints, seeds
# ---------------------------------------------------------------------------------------------
SHAPES = [(70, 61), (61,), (4100,), (9, 5)]


def _make(gpu, dt, groups=1, **kw):
    from zero_amd import zero2

    g0 = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter((torch.randn(s, generator=g0) * 0.1).to(dt).to(gpu)) for s in SHAPES]
    pg = params if groups == 1 else [{"params": params[:2]}, {"params": params[2:], "lr": 3e-3}]
    return params, zero2.ShardedOptimizer(torch.optim.Adam(pg, lr=1e-3), **{**SR, **kw})


def _run(gpu, params, opt, t0, t1, skip=lambda t, i: False):
    for t in range(t0, t1):
        opt.zero_grad()
        bt._inject(gpu, params, t)
        for i, p in enumerate(params):
            if skip(t, i):
                p.grad = None
        opt.step()
    torch.cuda.synchronize()


def test_two_groups_at_different_step_counts(gpu, pg1):
    """The second group's parameters get their first gradient a step late: their launches are
    keyed by their own step count, one behind the first group's."""
    params, opt = _make(gpu, BF16, groups=2, state_seed=SEED)
    ref = [_Ref(host(p)) for p in params]
    _bind2(opt, ref)
    late = lambda t, i: t == 0 and i >= 2  # noqa: E731
    for t in range(4):
        opt.zero_grad()
        bt._inject(gpu, params, t)
        grads = [None if late(t, i) else host(p.grad) for i, p in enumerate(params)]
        for i, p in enumerate(params):
            if late(t, i):
                p.grad = None
        opt.step()
        for i, (p, r, g) in enumerate(zip(params, ref, grads)):
            if g is not None:
                r.step(g, lr=1e-3 if i < 2 else 3e-3)
            if r.t:
                r.check(p, opt.optimizer.state[p], f"step {t} param {i}")
    assert [r.t for r in ref] == [4, 4, 3, 3] == [int(s) for s in opt.engine.steps]


def test_checkpoint_continues_the_saved_runs_bits(gpu, pg1):
    """Save after step 2, load into a fresh optimizer built with another seed: it adopts the saved
    seed, and steps 3 and 4 equal the uninterrupted run's bits."""
    pa, oa = _make(gpu, BF16, state_seed=11)
    _run(gpu, pa, oa, 0, 4)
    pb, ob = _make(gpu, BF16, state_seed=11)
    _run(gpu, pb, ob, 0, 2)
    ck = bt._roundtrip({"params": [p.detach().cpu() for p in pb], "opt": ob.state_dict()})
    assert ck["opt"]["zero_amd"]["state_seed"] == 11
    pc, oc = _make(gpu, BF16, state_seed=99)
    with torch.no_grad():
        for p, saved in zip(pc, ck["params"]):
            p.copy_(saved)
    oc.load_state_dict(ck["opt"])
    assert oc.state_seed == oc.engine.state_seed == 11
    _run(gpu, pc, oc, 2, 4)
    for i, (a, c) in enumerate(zip(pa, pc)):
        _same(host(c), host(a), f"param {i}")
        for name in ("exp_avg", "exp_avg_sq", "master_residual"):
            _same(host(oc.optimizer.state[c][name]), host(oa.optimizer.state[a][name]), f"{name} {i}")
    # a checkpoint written without the option loads as before and keeps this optimizer's seed
    pd, od = _make(gpu, BF16, state_seed=5)
    plain = oa.state_dict()
    del plain["zero_amd"]["state_seed"]
    od.load_state_dict(plain)
    assert od.state_seed == od.engine.state_seed == 5


def test_seeds(gpu, pg1):
    """Two seeds give different moment bits, one seed the same bits on a rerun."""
    out = []
    for seed in (1, 2, 1):
        params, opt = _make(gpu, BF16, state_seed=seed)
        _run(gpu, params, opt, 0, 2)
        out.append([np.concatenate([host(opt.optimizer.state[p][k]) for p in params])
                    for k in ("exp_avg", "exp_avg_sq")])
    for k in range(2):
        assert np.array_equal(out[0][k], out[2][k])
        assert (out[0][k] != out[1][k]).mean() > 0.1


# ---------------------------------------------------------------------------------------------
# ZeRO-3 in update mode (probe modules: the gradient of a weight is its coefficient, bit for bit)
# ---------------------------------------------------------------------------------------------
def _build3(dev, comm, **kw):
    from zero_amd import zero3

    init = z3t._init_weights("bf16")
    model = ProbeModel([Probe(torch.from_numpy(w.copy()).to(dev, BF16)) for w in init])
    params = [m.weight for m in model.probes]
    if comm is not None:
        kw["comm"] = comm
    opt = zero3.ShardedOptimizer(torch.optim.Adam(params, lr=z3t.LR), update=True, state_seed=SEED,
                                 bucket_mb=z3t.BUCKET_MB, **SR, **kw)
    zero3.register_zero3_hooks(model, opt.param_managers)
    return model, params, opt, [_Ref(zo.f32_to_bf16_bits(w)) for w in init]


def _zero3_schedule(rank, ws, dev, comm, passes, nsum=None, **kw):
    """One step per entry of ``passes`` (backward passes in it; two or more: the fp32 arena).
    Returns the optimizer and how many steps went through ``run_parts`` (the others took the
    cached sets)."""
    nsum = nsum or ws
    model, params, opt, ref = _build3(dev, comm, **kw)
    core = opt._core
    assert core.state_rounding == "stochastic" and core.state_seed == SEED
    for i, r in enumerate(ref):  # this rank's rows lie at the arena slot; the others are not checked
        n = int(np.prod(z3t.SHAPES[i]))
        mine = _rows(np.arange(n), z3t.SHAPES[i], ws, rank)
        assert mine.size == int(opt._arena.ln[i])
        r.e = np.zeros(n, np.uint64)
        r.e[mine] = int(opt._arena.slot[i]) + np.arange(mine.size, dtype=np.uint64)
    general, run_parts = [0], core.run_parts

    def counted(*a, **k):
        general[0] += 1
        return run_parts(*a, **k)

    core.run_parts = counted
    for step, npass in enumerate(passes):
        chunks = [[] for _ in params]
        for pas in range(npass):
            z3t._backward(model, step, pas, rank, dev)
            for i in range(len(params)):
                chunks[i].append(z3t.delivered(step, pas, i, nsum))
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        for i, (p, r) in enumerate(zip(params, ref)):
            acc = a32.accumulate_passes(chunks[i]) if ws > 1 else \
                zo.f32_to_bf16_bits(a32.exact_sum(chunks[i]).astype(np.float32))
            r.step(acc, div=float(ws), lr=z3t.LR)
            st = opt.optimizer.state[p]
            assert (st["exp_avg"].data_ptr() - core.m.data_ptr()) // 2 == int(opt._arena.slot[i])
            r.check(p, st, f"rank {rank} step {step} param {i}",
                    rows=lambda a, i=i: _rows(a, z3t.SHAPES[i], ws, rank))
    return opt, general[0]


def test_ws1_zero3_update_mode(gpu, pg1):
    opt, _ = _zero3_schedule(0, 1, gpu, None, (1, 1, 1, 1))
    assert opt._core.last_adam_bytes == 18 * sum(p.numel() for p in opt.params)


@pytest.fixture
def sim2(pg1, monkeypatch):
    import zero_amd.zero3 as z3

    real_get = z3.get
    monkeypatch.setattr(z3, "get", lambda what, dm=None: {"ws": 2, "rank": 0}[what]
                        if what in ("ws", "rank") else real_get(what, dm))
    yield


def test_simulated_ws2_zero3_takes_the_cached_sets(gpu, sim2):
    """Rank 0 of a simulated two-rank job, one pass per step: the first step builds the sets, the
    three after it launch the cached ones with that step's keys."""
    from _gloo_comm import SimRankComm

    opt, general = _zero3_schedule(0, 2, gpu, SimRankComm(2, 0), (1, 1, 1, 1), nsum=1)
    assert general == 1 and opt._fast_sets.get(False)


def test_simulated_ws2_zero3_fp32_accumulation(gpu, sim2):
    """Two accumulation passes under accumulation_dtype=torch.float32: the fp32-gradient
    split-master instance, alternating with the bf16-gradient one."""
    from _gloo_comm import SimRankComm

    opt, general = _zero3_schedule(0, 2, gpu, SimRankComm(2, 0), (2, 1, 2, 1), nsum=1,
                                   grad_accumulation=True, accumulation_dtype=torch.float32)
    assert opt._acc_widen and {ck[3] for ck in opt._adam_cache} == {False, True}
    assert general == 2


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_constructor_refusals(gpu, pg1):
    from zero_amd import zero1, zero2, zero3

    P = lambda: [torch.nn.Parameter(torch.zeros(8, device=gpu))]  # noqa: E731
    adam = lambda **kw: torch.optim.Adam(P(), lr=1e-3, **kw)  # noqa: E731
    for mk in (zero1.ShardedOptimizer, zero2.ShardedOptimizer,
               lambda o, **kw: zero3.ShardedOptimizer(o, update=True, **kw)):
        with pytest.raises(ValueError, match="state_dtype=torch.bfloat16"):
            mk(adam(), state_rounding="stochastic")  # fp32 state
        with pytest.raises(ValueError, match="state_dtype=torch.bfloat16"):
            mk(adam(), state_dtype=torch.float32, state_rounding="stochastic")
        with pytest.raises(ValueError, match="SGD"):
            mk(torch.optim.SGD(P(), lr=0.1, momentum=0.9), **SR)
        with pytest.raises(ValueError, match="state_rounding"):
            mk(adam(), state_dtype=BF16, state_rounding="random")
        for seed in (-1, 1 << 64, 0.5):
            with pytest.raises(ValueError, match="state_seed"):
                mk(adam(), state_seed=seed, **SR)
        with pytest.raises(ValueError, match="amsgrad"):
            mk(adam(amsgrad=True), **SR)
        # the default rounding keeps its bound and its message
        for rounding in (None, "nearest"):
            with pytest.raises(ValueError, match=r"beta2.*0\.99609375"):
                mk(adam(), state_dtype=BF16, state_rounding=rounding)
    for mod in (zero1, zero2):
        opt = mod.ShardedOptimizer(adam(), **SR)  # torch's default betas: accepted
        assert opt.state_rounding == "stochastic" and opt.state_seed == 0
        near = mod.ShardedOptimizer(adam(betas=(0.9, 0.95)), state_dtype=BF16)
        assert near.state_rounding == "nearest" and "state_seed" not in near.state_dict()["zero_amd"]
    with pytest.raises(ValueError, match="update"):
        zero3.ShardedOptimizer(adam(), update=False, **SR)
    with pytest.raises(ValueError, match="bucket"):
        zero2.ShardedOptimizer(adam(), arena="buckets", **SR)


# ---------------------------------------------------------------------------------------------
# world size 2 through real RCCL
# ---------------------------------------------------------------------------------------------
def _ws2_zero2_worker(rank, ws, port):
    """ZeRO-2 on the flat arena, bf16 split master, several rounds (4,096-element windows): each
    owner's launches draw from the indices of its own shard."""
    from _gloo_comm import test_comm
    from zero_amd import zero2

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    shapes = [(100, 91), (63,), (4096 + 41,), (7, 3)]
    rng = np.random.default_rng(17)
    bits = lambda s, scale: zo.f32_to_bf16_bits((rng.standard_normal(s) * scale).astype(np.float32)).reshape(-1)  # noqa: E731
    init = [bits(s, 0.05) for s in shapes]
    dev_bf16 = lambda b, s: torch.from_numpy(b.view(np.int16).copy()).view(BF16).reshape(s).to(dev)  # noqa: E731
    params = [torch.nn.Parameter(dev_bf16(a, s)) for a, s in zip(init, shapes)]
    ref = [_Ref(a) for a in init]
    local = [[[bits(s, 1e-2) for s in shapes] for _ in range(ws)] for _ in range(4)]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), comm=test_comm(),
                                 bucket_mb=ws * 4096 * 2 / (1 << 20), state_seed=SEED, **SR)
    assert opt.engine.split and opt.engine.K > 1 and opt.state_rounding == "stochastic"
    _bind2(opt, ref)
    for t in range(4):
        opt.zero_grad()
        for p, g, s in zip(params, local[t][rank], shapes):
            set_grad(p, dev_bf16(g, s))
        opt.step()
        for i, (p, r) in enumerate(zip(params, ref)):
            red = zo.f32_to_bf16_bits(zo.bf16_bits_to_f32(local[t][0][i]) + zo.bf16_bits_to_f32(local[t][1][i]))
            r.step(red, div=2.0)
            st = opt.optimizer.state[p] if i in opt.local_param_indices else None
            r.check(p, st, f"rank {rank} step {t} param {i}")
    dist.barrier()
    dist.destroy_process_group()


def _ws2_zero1_refused_worker(rank, ws, port):
    """ZeRO-1 at world size 2 keeps the gradient carry: refused as without the option."""
    from zero_amd import zero1

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    p = torch.nn.Parameter(torch.zeros(8, device="cuda:0"))
    with pytest.raises(ValueError, match="ZeRO-1"):
        zero1.ShardedOptimizer(torch.optim.Adam([p], lr=1e-3), **SR)
    dist.destroy_process_group()


def test_ws2_rccl(gpu, rccl_env):
    t0 = time.perf_counter()
    spawn_batch(2, [(_ws2_zero2_worker, ()), (_ws2_zero1_refused_worker, ())], all_spawned=True)
    print(f"ws=2 stochastic-rounding batch: {time.perf_counter() - t0:.1f} s")
