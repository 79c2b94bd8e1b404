"""``ShardedOptimizer(..., master="none")`` behind ZeRO-1 and ZeRO-2 on the flat arena: bf16
parameters without any master, updated in place and rounded stochastically.

Every trajectory is compared bit for bit with the restatement of tests/_psr_oracle.py, driven with
the shard indices the engine uses (from its plan, checked against where the state views lie), the
optimizer's seed and each parameter's own step count.  World size 2 runs through real RCCL in one
batch: the parameters after the broadcast are the same on both ranks and equal the oracle.
"""
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist

import _psr_oracle as po
import test_gpu_bf16_state_optimizer as bt
from _zero_run import init_pg, set_grad, spawn_batch
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_clip_optimizer import pg1, rccl_env  # noqa: F401

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
BETAS = (0.9, 0.95)  # inside the bound that bf16 moments rounded to nearest need
SEED = (0xABCDEF << 32) | 0x13579B
STATE_KW = {"f32": {}, "bf16": dict(state_dtype=BF16),
            "bf16_sr": dict(state_dtype=BF16, state_rounding="stochastic")}
BYTES = {"f32": 22, "bf16": 14, "bf16_sr": 14}
host, _same = bt.host, bt._same


class _Ref:
    """One bf16 parameter under the restatement; ``e``: its elements' shard indices."""

    def __init__(self, init_bits, state, seed=SEED, **hp):
        self.p = np.ascontiguousarray(init_bits, np.uint16).reshape(-1).copy()
        z = np.float32 if state == "f32" else np.uint16
        self.m, self.v = np.zeros(self.p.size, z), np.zeros(self.p.size, z)
        self.state, self.seed, self.hp, self.t, self.e = state, seed, hp, 0, None

    def step(self, g_bits, div=1.0, coef=None):
        self.t += 1
        g = np.ascontiguousarray(g_bits).reshape(-1)
        if coef is not None:  # the unchanged step on the pre-clipped gradient
            gf = zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g
            with np.errstate(all="ignore"):
                g = np.ascontiguousarray((gf / np.float32(div)).astype(np.float32) * np.float32(coef))
            div = 1.0
        chp = c_oracle.hparams(step=self.t, grad_div=float(div), beta1=BETAS[0], beta2=BETAS[1],
                               **self.hp)
        po.step(self.p, g, self.m, self.v, chp, np.asarray(self.e, np.uint64),
                po.keys_of(self.seed, self.t), self.state)

    def check(self, p, st, what, rows=lambda a: a):
        """``st``: optimizer.state[p] (None: a parameter this rank does not own)."""
        _same(host(p), rows(self.p), what + " param")
        if st is None:
            return
        assert "master_param" not in st and "master_residual" not in st, what
        sdt = torch.float32 if self.state == "f32" else BF16
        assert st["exp_avg"].dtype == sdt and st["exp_avg_sq"].dtype == sdt
        assert st["exp_avg"].shape == p.shape
        _same(host(st["exp_avg"]), rows(self.m), what + " exp_avg")
        _same(host(st["exp_avg_sq"]), rows(self.v), what + " exp_avg_sq")


def _offsets(opt):
    """param index -> offset of its state in its owner's shard, from the engine's plan; the owned
    ones are checked against where their exp_avg view lies in the shard's m array."""
    eng, off = opt.engine, {}
    for r in range(opt.world_size):
        pc = eng.plan.pieces(r)
        for i, o, s, n in zip(pc.param.tolist(), pc.param_off.tolist(), pc.stream_off.tolist(),
                              pc.length.tolist()):
            if n > 0:
                assert o == 0 and n == opt.params[i].numel()
                off[i] = s
    for i in opt.local_param_indices:
        st = opt.optimizer.state[opt.params[i]]
        assert (st["exp_avg"].data_ptr() - eng.m.data_ptr()) // eng.m.element_size() == off[i]
    return off


def _bind(opt, ref):
    off = _offsets(opt)
    for i, r in enumerate(ref):
        r.e = off[i] + np.arange(opt.params[i].numel(), dtype=np.uint64)


# ---------------------------------------------------------------------------------------------
# world size 1 through a real backward: two groups, one parameter that never gets a gradient
# ---------------------------------------------------------------------------------------------
GROUP_HP = (dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-3, weight_decay=1e-2))


def _mlp(gpu):
    """96 x 97 = two chunks of 4,096 and a partial one, 97 = 96 + a one-element scalar tail,
    97 x 7 = 676 + a three-element one; ``idle`` requires a gradient and never receives one."""
    torch.manual_seed(0)
    mk = lambda *s: torch.nn.Parameter((torch.randn(*s) * 0.1).to(BF16).to(gpu))  # noqa: E731
    w1, b1, w2, idle = mk(96, 97), mk(97), mk(97, 7), mk(33)
    x, y = torch.randn(32, 96).to(BF16).to(gpu), torch.randn(32, 7).to(BF16).to(gpu)
    loss = lambda: (((torch.tanh(x @ w1 + b1) @ w2) - y) ** 2).sum()  # noqa: E731
    groups = [dict(params=[w1, b1], **GROUP_HP[0]), dict(params=[w2, idle], **GROUP_HP[1])]
    return [w1, b1, w2, idle], groups, loss


CASES = [("zero2", "f32", False), ("zero2", "bf16", False), ("zero2", "bf16_sr", False),
         ("zero2", "bf16_sr", True), ("zero1", "bf16_sr", False), ("zero1", "f32", True)]


@pytest.mark.parametrize("variant,state,clip", CASES)
def test_ws1_through_backward(gpu, pg1, variant, state, clip):
    from zero_amd import zero1, zero2

    mod = {"zero1": zero1, "zero2": zero2}[variant]
    params, groups, loss = _mlp(gpu)
    ref = [_Ref(host(p), state, **GROUP_HP[i // 2]) for i, p in enumerate(params)]
    opt = mod.ShardedOptimizer(torch.optim.Adam(groups, betas=BETAS), master="none",
                               state_seed=SEED, max_grad_norm=1.0 if clip else None,
                               **STATE_KW[state])
    eng = opt.engine
    assert eng.master_free and eng.master is None and eng.lo is None and not eng.split
    assert opt.state_seed == eng.state_seed == SEED
    _bind(opt, ref)
    idle0 = host(params[3])
    stepped = sum(p.numel() for p in params[:3])
    for t in range(1, 6):
        opt.zero_grad()
        (loss() * (1.0, 40.0, 0.05, 1.0, 1.0)[t - 1]).backward()
        assert params[3].grad is None
        grads = [host(p.grad) for p in params[:3]]
        coef = None
        if clip and t == 1:
            sq = sum(float(np.sum(zo.bf16_bits_to_f32(g).astype(np.float64) ** 2)) for g in grads)
            opt.max_grad_norm = 4.0 * np.sqrt(sq)  # coefficients: 1, about 0.1, 1, 1, 1
        opt.step()
        if clip:
            coef = np.float32(opt.last_clip_coef.item())
            assert (coef == 1.0) == (t != 2) and (t != 2 or 0.05 < coef < 0.2)
        assert eng.last_adam_bytes == BYTES[state] * stepped
        for i, (p, r, g) in enumerate(zip(params, ref, grads)):
            r.step(g, coef=coef)
            r.check(p, opt.optimizer.state[p], f"step {t} param {i}")
            assert int(opt.optimizer.state[p]["step"].item()) == t
    assert np.array_equal(host(params[3]), idle0) and int(eng.steps[3]) == 0
    assert not opt.optimizer.state[params[3]]["exp_avg"].any()


# ---------------------------------------------------------------------------------------------
# injected gradients: checkpoints, seeds, the memory report
# ---------------------------------------------------------------------------------------------
SHAPES = [(70, 61), (61,), (4100,), (9, 5)]


def _make(gpu, **kw):
    from zero_amd import zero2

    g0 = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter((torch.randn(s, generator=g0) * 0.1).to(BF16).to(gpu))
              for s in SHAPES]
    kw = {"master": "none", **kw}
    return params, zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3, betas=BETAS), **kw)


def _run(gpu, params, opt, t0, t1):
    for t in range(t0, t1):
        opt.zero_grad()
        bt._inject(gpu, params, t)
        opt.step()
    torch.cuda.synchronize()


def _load_params(dst, saved):
    with torch.no_grad():
        for p, s in zip(dst, saved):
            p.copy_(s)


@pytest.mark.parametrize("state", ["f32", "bf16_sr"])
def test_checkpoint_round_trip(gpu, pg1, state):
    """Save after step 2, load into a fresh optimizer built with another seed: it adopts the saved
    seed, and steps 3 to 5 equal the uninterrupted run's bits."""
    kw = STATE_KW[state]
    pa, oa = _make(gpu, state_seed=11, **kw)
    _run(gpu, pa, oa, 0, 5)
    pb, ob = _make(gpu, state_seed=11, **kw)
    _run(gpu, pb, ob, 0, 2)
    ck = bt._roundtrip({"params": [p.detach().cpu() for p in pb], "opt": ob.state_dict()})
    head = ck["opt"]["zero_amd"]
    assert head["master"] == "none" and head["state_seed"] == 11
    for entry in ck["opt"]["state"].values():
        assert sorted(entry) == ["exp_avg", "exp_avg_sq", "step"]
    pc, oc = _make(gpu, state_seed=99, **kw)
    _load_params(pc, ck["params"])
    oc.load_state_dict(ck["opt"])
    assert oc.state_seed == oc.engine.state_seed == 11
    _run(gpu, pc, oc, 2, 5)
    for i, (a, c) in enumerate(zip(pa, pc)):
        _same(host(c), host(a), f"param {i}")
        assert sorted(oc.optimizer.state[c]) == ["exp_avg", "exp_avg_sq", "step"]
        for name in ("exp_avg", "exp_avg_sq"):
            _same(host(oc.optimizer.state[c][name]), host(oa.optimizer.state[a][name]), f"{name} {i}")


def test_checkpoints_between_masters(gpu, pg1):
    """A checkpoint that carries a master (the split master's residual, the fp32 master) is
    refused by master="none": it would drop the master's precision without a word.  The other way
    round loads, the residual starting at 0."""
    for master, key in (("split", "master_residual"), ("fp32", "master_param")):
        ps, osrc = _make(gpu, master=master)
        _run(gpu, ps, osrc, 0, 2)
        sd = bt._roundtrip(osrc.state_dict())
        assert sd["zero_amd"]["master"] == master and key in sd["state"][0]
        pn, on = _make(gpu)
        before = [host(on.optimizer.state[p]["exp_avg"]) for p in pn]
        with pytest.raises(ValueError, match=key):
            on.load_state_dict(sd)
        for p, b in zip(pn, before):  # (refused before anything was copied)
            assert np.array_equal(host(on.optimizer.state[p]["exp_avg"]), b)
    pn, on = _make(gpu, state_seed=4)
    _run(gpu, pn, on, 0, 2)
    sd = bt._roundtrip(on.state_dict())
    psp, osp = _make(gpu, master="split")
    _load_params(psp, [p.detach().cpu() for p in pn])
    osp.load_state_dict(sd)
    for a, b in zip(pn, psp):
        sa, sb = on.optimizer.state[a], osp.optimizer.state[b]
        assert not sb["master_residual"].any() and int(sb["step"].item()) == 2
        _same(host(sb["exp_avg"]), host(sa["exp_avg"]), "exp_avg")
    _run(gpu, psp, osp, 2, 3)  # and steps on


def test_seeds(gpu, pg1):
    """One seed gives the same bits on a rerun; state_seed = 1 gives other parameters after one
    step — with fp32 moments too, where the seed keys the parameter's draw alone."""
    for state in ("f32", "bf16_sr"):
        out = []
        for seed in (0, 1, 0):
            params, opt = _make(gpu, state_seed=seed, **STATE_KW[state])
            _run(gpu, params, opt, 0, 1)
            out.append(np.concatenate([host(p) for p in params]))
        assert np.array_equal(out[0], out[2]), state
        assert (out[0] != out[1]).mean() > 0.1, state


def test_memory_report_shows_6_bytes_per_parameter(gpu, pg1):
    from zero_amd.training_utils.memory import memory_report

    class Model:
        def __init__(self, params):
            self.params = params

        def parameters(self):
            return iter(self.params)

    n = sum(int(np.prod(s)) for s in SHAPES)
    per = {}
    for name, kw in (("none", dict(master="none")), ("split", dict(master="split"))):
        params, opt = _make(gpu, **{**STATE_KW["bf16_sr"], **kw})
        _run(gpu, params, opt, 0, 1)
        rep = memory_report(Model(params), opt, gpu)
        per[name] = (rep.params_mb + rep.optimizer_mb) * (1 << 20) / n
    print("bytes per parameter, parameters + optimizer state:", per)
    assert abs(per["none"] - 6.0) < 0.01 and abs(per["split"] - 8.0) < 0.01


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_constructor_refusals(gpu, pg1):
    """ValueError at construction, before the engine or a communicator exists."""
    from zero_amd import zero1, zero2

    def P(dtype=BF16):
        return [torch.nn.Parameter(torch.zeros(8, 8, dtype=dtype, device=gpu))]

    adam = lambda **kw: torch.optim.Adam(P(), lr=1e-3, **kw)  # noqa: E731
    for mod in (zero1, zero2):
        cases = [(lambda: torch.optim.Adam(P(torch.float32)), {}, "bf16 parameters"),
                 (lambda: torch.optim.SGD(P(), lr=0.1, momentum=0.9), {}, "SGD"),
                 (lambda: adam(amsgrad=True), {}, "amsgrad"),
                 (adam, dict(arena="buckets"), "bucket arena"),
                 (adam, dict(layout="zero"), "bucket arena"),
                 (adam, dict(overlap=True), "overlap"),
                 (adam, dict(state_seed=-1), "state_seed"),
                 (adam, dict(state_seed=1 << 64), "state_seed")]
        for mk, kw, word in cases:
            with pytest.raises(ValueError, match=word):
                mod.ShardedOptimizer(mk(), master="none", **kw)
        with pytest.raises(ValueError, match="master must be"):
            mod.ShardedOptimizer(adam(), master="half")
    # amsgrad switched on between steps is refused at the step, as bf16 state refuses it
    params = P()
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), master="none")
    params[0].grad = torch.ones_like(params[0])
    opt.step()
    opt.optimizer.param_groups[0]["amsgrad"] = True
    before = host(params[0])
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    torch.cuda.synchronize()
    assert np.array_equal(host(params[0]), before)


# ---------------------------------------------------------------------------------------------
# world size 2 through real RCCL
# ---------------------------------------------------------------------------------------------
def _ws2_zero2_worker(rank, ws, port, state):
    """ZeRO-2 on the flat arena, several rounds (4,096-element windows): each owner's launches
    draw from the indices of its own shard, and the broadcast hands every rank the same bits."""
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
    ref = [_Ref(a, state, lr=1e-3) for a in init]
    local = [[[bits(s, 1e-2) for s in shapes] for _ in range(ws)] for _ in range(5)]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3, betas=BETAS), comm=test_comm(),
                                 bucket_mb=ws * 4096 * 2 / (1 << 20), state_seed=SEED,
                                 master="none", **STATE_KW[state])
    assert opt.engine.master_free and opt.engine.K > 1
    _bind(opt, ref)
    for t in range(5):
        opt.zero_grad()
        for p, g, s in zip(params, local[t][rank], shapes):
            set_grad(p, dev_bf16(g, s))
        opt.step()
        for i, (p, r) in enumerate(zip(params, ref)):
            red = zo.f32_to_bf16_bits(zo.bf16_bits_to_f32(local[t][0][i]) + zo.bf16_bits_to_f32(local[t][1][i]))
            r.step(red, div=2.0)
            st = opt.optimizer.state[p] if i in opt.local_param_indices else None
            r.check(p, st, f"rank {rank} step {t} param {i}")
    every = [None] * ws  # the same bits on both ranks
    dist.all_gather_object(every, [host(p).tobytes() for p in params])
    assert every[0] == every[1]
    dist.barrier()
    dist.destroy_process_group()


def _ws2_zero1_refused_worker(rank, ws, port):
    """ZeRO-1 at world size 2 keeps the gradient carry: refused on every rank."""
    from zero_amd import zero1

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    p = torch.nn.Parameter(torch.zeros(8, dtype=BF16, device="cuda:0"))
    with pytest.raises(ValueError, match="carry"):
        zero1.ShardedOptimizer(torch.optim.Adam([p], lr=1e-3), master="none")
    dist.destroy_process_group()


def test_ws2_rccl(gpu, rccl_env):
    t0 = time.perf_counter()
    spawn_batch(2, [(_ws2_zero2_worker, ("bf16_sr",)), (_ws2_zero2_worker, ("f32",)),
                    (_ws2_zero1_refused_worker, ())], all_spawned=True)
    print(f"ws=2 master-free batch: {time.perf_counter() - t0:.1f} s")
