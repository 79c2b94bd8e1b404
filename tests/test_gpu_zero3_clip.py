"""``zero3.ShardedOptimizer(update=True, max_grad_norm=...)``: global gradient-norm clipping over
the chunks each rank updates, at world size 1, at simulated ranks (SimRankComm: the other ranks
contribute zeros, and nothing to the norm) and at world size 2 through real RCCL.

Gradients are known exactly (tests/_clip_inputs.py: probe modules whose gradient is a planted
coefficient tensor), three steps scaled x1, x40 and x0.05 with ``max_grad_norm`` four times the
first step's norm: the coefficients are exactly 1, about 0.1 and exactly 1 (Adam's update is nearly
invariant to the gradient's scale, so the state is compared too).  fp32 parameters follow a CPU
replica (``clip_grad_norm_`` + ``torch.optim.AdamW`` on the averaged gradient) to 1e-6 relative, the
bound of tests/test_gpu_clip_optimizer.py; every other case equals its oracle bit for bit, fed the
pre-clipped gradient with the coefficient the device reported.
"""
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist

import _bf16_state_oracle as bo
import _bf16_state_sr_oracle as sro
import _clip_inputs as ci
import _sgd_oracle as so
from _zero_run import init_pg, rel, spawn_batch
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_clip_optimizer import _Replica, pg1, rccl_env  # noqa: F401
from test_gpu_zero3_accumulate import Probe, ProbeModel, _chunk, _rows

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
ADAM = dict(lr=1e-3, betas=(0.9, 0.95))
HP = dict(lr=1e-3, beta1=0.9, beta2=0.95)
SGD = dict(lr=0.05, momentum=0.9)
SEED = (0xABCDEF << 32) | 0x13579B
BUCKET_MB = 0.02  # (66, 128) is a bucket of its own: two buckets per pass
ONE = 0x3F800000
STATE_KW = {"f32": {}, "bf16": dict(state_dtype=BF16),
            "sr": dict(state_dtype=BF16, state_rounding="stochastic", state_seed=SEED)}


def host(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().view(np.uint32).copy()


def _same(got, want, what):
    want = np.ascontiguousarray(want).reshape(-1)
    want = want.view(np.uint32) if want.dtype == np.float32 else want
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:6]}"


def _f32(t):
    return np.float32(t.item())


def _init_weights(pdt, shapes):
    rng = np.random.default_rng(3)
    out = []
    for s in shapes:
        w = (rng.standard_normal(s) * 0.1).astype(np.float32)
        if pdt == "bf16":
            w = zo.bf16_bits_to_f32(zo.f32_to_bf16_bits(w)).reshape(s)
        out.append(w)
    return out


def _build(dev, pdt, comm, shapes, inner=None, **kw):
    from zero_amd import zero3

    init = _init_weights(pdt, shapes)
    tdt = torch.float32 if pdt == "f32" else BF16
    model = ProbeModel([Probe(torch.from_numpy(w.copy()).to(dev, tdt)) for w in init])
    params = [m.weight for m in model.probes]
    inner = torch.optim.Adam(params, **ADAM) if inner is None else inner(params)
    if comm is not None:
        kw["comm"] = comm
    opt = zero3.ShardedOptimizer(inner, update=True, bucket_mb=BUCKET_MB, **kw)
    zero3.register_zero3_hooks(model, opt.param_managers)
    return model, params, opt, init


def _backward(model, step, pas, rank, arena, dev, shapes, on=None):
    for k, m in enumerate(model.probes):
        m.c = torch.from_numpy(ci.local(step, pas, rank, k, arena, shapes)).to(dev, m.weight.dtype)
    model([True] * len(shapes) if on is None else on).backward()


class _Ref:
    """This rank's rows of one parameter under the oracle of its configuration."""

    def __init__(self, rows, pdt, state, sgd, slot):
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        self.split, self.state, self.sgd, self.t = pdt == "bf16", state, sgd, 0
        if self.split:
            self.hi, self.lo = zo.f32_to_bf16_bits(rows), np.zeros(rows.size, np.uint16)
        else:
            self.p = rows.copy()
        sdt = np.float32 if state == "f32" else np.uint16
        self.m, self.v = np.zeros(rows.size, sdt), np.zeros(rows.size, sdt)
        self.e = np.uint64(slot) + np.arange(rows.size, dtype=np.uint64)

    def step(self, g, div, coef):
        """``g``: the gradient sum the update reads (bf16 bits or fp32), ``coef`` the device's."""
        self.t += 1
        g = np.ascontiguousarray(g).reshape(-1)
        gf = zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g
        if self.sgd:
            hp = so.SgdHP(SGD["lr"], SGD["momentum"], first=self.t == 1, grad_div=float(div))
            self.p, self.m, _ = so.sgd_elem(gf, self.p, None if self.t == 1 else self.m, hp,
                                            coef=np.float32(coef))
            return
        with np.errstate(all="ignore"):  # the unchanged fp32 step on the pre-clipped gradient
            gp = np.ascontiguousarray((gf / np.float32(div)).astype(np.float32) * np.float32(coef))
        chp = c_oracle.hparams(step=self.t, grad_div=1.0, **HP)
        p = c_oracle.join_master(self.hi, self.lo) if self.split else self.p
        if self.state == "f32":
            c_oracle.adam_f32(p, gp, self.m, self.v, chp)
        elif self.state == "bf16":
            bo.adam_f32(p, gp, self.m, self.v, chp)
        else:
            sro.adam_f32(p, gp, self.m, self.v, chp, self.e, sro.keys_of(SEED, self.t))
        if self.split:
            self.hi, self.lo = c_oracle.split_master(p)

    def check(self, p, st, what):
        _same(host(p), self.hi if self.split else self.p, what + " param")
        if self.split:
            _same(host(st["master_residual"]), self.lo, what + " residual")
        if self.sgd:
            _same(host(st["momentum_buffer"]), self.m, what + " buffer")
            return
        _same(host(st["exp_avg"]), self.m, what + " exp_avg")
        _same(host(st["exp_avg_sq"]), self.v, what + " exp_avg_sq")


def _coef_of(norm, limit):
    """min(1, f32(m) / (norm + f32(1e-6))) in fp32 from the reported norm, as bits."""
    with np.errstate(all="ignore"):
        c = np.float32(limit) / np.float32(np.float32(norm) + np.float32(1e-6))
    return (np.float32(1.0) if c > np.float32(1.0) else np.float32(c)).view(np.uint32)


def _check_reported(opt, want_norm, limit, ws, real, what):
    norm, coef = _f32(opt.last_grad_norm), _f32(opt.last_clip_coef)
    assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.dtype == torch.float32
    print(f"{what}: norm {norm!r} vs float64 {want_norm!r}, coef {coef!r}")
    assert abs(float(norm) - want_norm) <= 1e-6 * want_norm, what
    assert coef.view(np.uint32) == _coef_of(norm, limit), what
    if real and ws > 1:
        every = [None] * ws
        dist.all_gather_object(every, int(norm.view(np.uint32)))
        assert len(set(every)) == 1, every
    return coef


def _norm64(grads, ws, rank, sim, shapes):
    """sqrt(sum g^2) / ws over the rows that enter: every rank's (the all-reduce), or -- at a
    simulated rank, whose peers contribute nothing -- this rank's alone."""
    sq = 0.0
    for i, g in enumerate(grads):
        if g is not None:
            v = ci.values(g)
            sq += float(np.sum((_rows(v, shapes[i], ws, rank) if sim else v) ** 2))
    return float(np.sqrt(sq)) / ws


def _case(rank, ws, dev, comm, pdt, state="f32", sgd=False, passes=1, acc32=False,
          side_stream=True, sim=False, shapes=ci.SHAPES):
    """Three clipped steps, bit for bit against the oracle of the configuration."""
    arena = "f32" if pdt == "f32" else "bf16"
    ranks = [rank] if sim or ws == 1 else list(range(ws))
    widen = acc32 and passes >= 2 and arena == "bf16" and ws > 1
    kw = dict(STATE_KW[state], side_stream=side_stream, max_grad_norm=1.0)
    if passes > 1:
        kw.update(grad_accumulation=True, accumulation_dtype=torch.float32 if acc32 else None)
    inner = (lambda ps: torch.optim.SGD(ps, **SGD)) if sgd else None
    model, params, opt, init = _build(dev, pdt, comm, shapes, inner, **kw)
    ar, core = opt._arena, opt._core
    ref = [_Ref(_rows(w, shapes[i], ws, rank), pdt, state, sgd, int(ar.slot[i]))
           for i, w in enumerate(init)]
    general, run_parts = [0], core.run_parts

    def counted(*a, **k):
        general[0] += 1
        return run_parts(*a, **k)

    core.run_parts = counted
    es = 4 if arena == "f32" or widen else 2
    coefs = []
    for step in range(len(ci.SCALES)):
        for pas in range(passes):
            _backward(model, step, pas, rank, arena, dev, shapes)
        grads = [ci.accumulated(step, passes, i, ranks, arena, widen, shapes)
                 for i in range(len(shapes))]
        norm = _norm64(grads, ws, rank, sim, shapes)
        if step == 0:
            # (a plain attribute: changed between steps; a simulated rank without elements: any)
            opt.max_grad_norm = 4.0 * norm if norm > 0 else 1.0
        opt.step()
        torch.cuda.synchronize()
        what = f"rank {rank} step {step}"
        if widen:
            assert opt._fast_sets.get(True) and opt._A is not None
        if norm > 0:
            coefs.append(_check_reported(opt, norm, opt.max_grad_norm, ws, not sim, what))
        else:  # (a simulated rank that updates nothing)
            assert _f32(opt.last_grad_norm) == 0.0
            coefs.append(_f32(opt.last_clip_coef))
        assert opt.last_norm_bytes == es * int(ar.ln.sum())
        for i, (p, r) in enumerate(zip(params, ref)):
            if int(ar.ln[i]) == 0:
                continue
            r.step(_rows(grads[i], shapes[i], ws, rank), float(ws), coefs[-1])
            r.check(p, opt.optimizer.state[p], f"{what} param {i}")
    print("coefficients", coefs)
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE
    if sum(int(np.prod(s)) for s in shapes) > 1:  # (one element: its three values are unrelated)
        assert 0.05 < coefs[1] < 0.2
    if ws > 1 and int(ar.ln.sum()):  # one step builds the sets, the others take the cached ones
        assert general[0] == 1 and opt._fast_sets.get(widen)
    return opt


def _replica(rank, ws, dev, comm, sim=False):
    """fp32, two AdamW groups, parameter 1 without a gradient in step 2 (the general partitioning
    path; torch leaves it out of the norm), against the CPU replica on the averaged gradient.

    The replica (``clip_grad_norm_`` + ``torch.optim.AdamW``) runs in float64: in fp32 torch's own
    norm of the 8,465 elements is 3.9e-6 off the float64 one in step 2, and through the
    coefficient its exp_avg_sq 7.8e-6 off a float64 replica's -- more than the 1e-6 the device is
    held to, so an fp32 replica cannot be the reference at that bound.  In float64 the replica's
    own error is below 1e-15 and the bound measures the device alone."""
    shapes = ci.SHAPES
    groups = [([0, 1], dict(lr=1e-3, weight_decay=1e-2)), ([2, 3], dict(lr=2e-3, weight_decay=0.0))]
    inner = lambda ps: torch.optim.AdamW([dict(params=[ps[i] for i in idx], **kw)  # noqa: E731
                                          for idx, kw in groups])
    model, params, opt, init = _build(dev, "f32", comm, shapes, inner, max_grad_norm=1.0)
    rep = _Replica([w.astype(np.float64) for w in init], groups)
    ar = opt._arena
    coefs = []
    for step in range(len(ci.SCALES)):
        on = [not (step == 1 and i == 1) for i in range(len(shapes))]
        _backward(model, step, 0, rank, "f32", dev, shapes, on)
        avg = []
        for i, s in enumerate(shapes):
            if not on[i]:
                avg.append(None)
            elif sim:  # the peers contribute zeros: this rank's rows alone are non-zero
                g = np.zeros(s, np.float32)
                _chunk(g, ws, rank)[...] = _chunk(ci.local(step, 0, rank, i, "f32"), ws, rank)
                avg.append(g / np.float32(ws))
            else:
                avg.append((ci.reduced(step, 0, i, list(range(ws)), "f32") / np.float32(ws)).reshape(s))
        if step == 0:
            opt.max_grad_norm = 4.0 * float(np.sqrt(sum(np.sum(g.astype(np.float64) ** 2) for g in avg)))
        opt.step()
        torch.cuda.synchronize()
        want = rep.step([None if g is None else g.astype(np.float64) for g in avg], opt.max_grad_norm)
        coefs.append(_check_reported(opt, want, opt.max_grad_norm, ws, not sim, f"rank {rank} step {step}"))
        assert opt.last_norm_bytes == 4 * sum(int(ar.ln[i]) for i in range(len(shapes)) if on[i])
        for i, p in enumerate(params):
            if int(ar.ln[i]) == 0:
                continue
            rows = lambda a: _rows(np.asarray(a), shapes[i], ws, rank)  # noqa: E731
            assert rel(p.detach().cpu().numpy().reshape(-1), rows(rep.params[i].detach().numpy())) <= 1e-6
            st = opt.optimizer.state[p]
            for name in ("exp_avg", "exp_avg_sq"):
                assert rel(st[name].cpu().numpy().reshape(-1), rows(rep.state(i, name))) <= 1e-6, (name, i)
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE and 0.05 < coefs[1] < 0.2


def _inf_equals_none(rank, ws, dev, comm, sim=False):
    """max_grad_norm=inf reports the norm and changes nothing: parameters and state bit-identical
    to the unclipped path over three steps, which allocates no clipping buffers."""
    out = {}
    for limit in (None, float("inf")):
        model, params, opt, _ = _build(dev, "bf16", comm, ci.SHAPES, max_grad_norm=limit)
        for step in range(len(ci.SCALES)):
            _backward(model, step, 0, rank, "bf16", dev, ci.SHAPES)
            opt.step()
            torch.cuda.synchronize()
            if limit is None:
                assert opt.last_grad_norm is None and opt.last_clip_coef is None
                assert opt._clip is None and opt.last_norm_bytes == 0 and opt.skipped_steps is None
            else:
                assert _f32(opt.last_clip_coef).view(np.uint32) == ONE
        out[limit] = [host(p) for p in params] + [host(opt._state)]
    for a, b in zip(out[None], out[float("inf")]):
        assert np.array_equal(a, b)


# ---- world size 1 -------------------------------------------------------------------------------
CONFIGS = [("f32", "f32", False), ("bf16", "f32", False), ("bf16", "bf16", False),
           ("bf16", "sr", False), ("f32", "f32", True)]
CONFIG_IDS = ["fp32", "split", "split-bf16state", "split-sr", "sgd"]


@pytest.mark.parametrize("pdt,state,sgd", CONFIGS, ids=CONFIG_IDS)
def test_ws1(gpu, pg1, pdt, state, sgd):
    _case(0, 1, gpu, None, pdt, state, sgd)


def test_ws1_replica_and_inf(gpu, pg1):
    _replica(0, 1, gpu, None)
    _inf_equals_none(0, 1, gpu, None)


def test_errors(gpu, pg1):
    from zero_amd import zero3

    P = lambda: [torch.nn.Parameter(torch.zeros(8, device=gpu))]  # noqa: E731
    with pytest.raises(ValueError, match="update mode"):
        zero3.ShardedOptimizer(torch.optim.Adam(P()), update=False, max_grad_norm=1.0)
    for bad in (-1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="max_grad_norm"):
            zero3.ShardedOptimizer(torch.optim.Adam(P()), update=True, max_grad_norm=bad)
    params = P()
    opt = zero3.ShardedOptimizer(torch.optim.Adam(params), update=True, max_grad_norm=1.0)
    for bad in (-1.0, float("nan"), "1"):
        opt.max_grad_norm = bad  # a limit set to a bad value between steps
        params[0].grad = torch.ones(8, device=gpu)
        with pytest.raises(ValueError, match="max_grad_norm"):
            opt.step()
    opt.max_grad_norm = 0.5
    opt.step()
    assert abs(float(opt.last_grad_norm.item()) - np.sqrt(8.0)) <= 1e-6 * np.sqrt(8.0)


# ---- simulated ranks ----------------------------------------------------------------------------
@pytest.fixture
def sim2(pg1, monkeypatch, request):
    import zero_amd.zero3 as z3

    rank = getattr(request, "param", 0)
    real_get = z3.get
    monkeypatch.setattr(z3, "get", lambda what, dm=None: {"ws": 2, "rank": rank}[what]
                        if what in ("ws", "rank") else real_get(what, dm))
    yield rank


@pytest.mark.parametrize("sim2", [0, 1], indirect=True)
@pytest.mark.parametrize("pdt,state,sgd", CONFIGS, ids=CONFIG_IDS)
def test_simulated_rank(gpu, sim2, pdt, state, sgd):
    from _gloo_comm import SimRankComm

    _case(sim2, 2, gpu, SimRankComm(2, sim2), pdt, state, sgd, sim=True)


@pytest.mark.parametrize("acc32", [False, True], ids=["bf16-arena", "fp32-arena"])
def test_simulated_rank_accumulation(gpu, sim2, acc32):
    """Two passes: the norm is that of the accumulated sum, over _A under accumulation_dtype=
    torch.float32 (the fp32-gradient split-master instances); single-stream mode too."""
    from _gloo_comm import SimRankComm

    for side in (True, False):
        opt = _case(0, 2, gpu, SimRankComm(2, 0), "bf16", passes=2, acc32=acc32, side_stream=side,
                    sim=True)
        assert opt.grad_arena().dtype == BF16  # (after step(): the bf16 arena again)
        assert (opt._A is not None) == acc32


def test_simulated_rank_replica_inf_and_empty(gpu, sim2):
    from _gloo_comm import SimRankComm

    _replica(0, 2, gpu, SimRankComm(2, 0), sim=True)
    _inf_equals_none(0, 2, gpu, SimRankComm(2, 0), sim=True)


@pytest.mark.parametrize("sim2", [1], indirect=True)
def test_simulated_rank_that_updates_nothing(gpu, sim2):
    """The model [(1,)] alone: rank 1's chunk has no element, it updates nothing, and every step
    reaches its end with norm 0 and coefficient 1."""
    from _gloo_comm import SimRankComm

    opt = _case(1, 2, gpu, SimRankComm(2, 1), "f32", sim=True, shapes=[(1,)])
    assert int(opt._arena.ln.sum()) == 0 and _f32(opt.last_clip_coef).view(np.uint32) == ONE


# ---- world size 2 through real RCCL --------------------------------------------------------------
def _mr(rank, ws, port, fn, *args):
    import faulthandler
    import sys

    from _gloo_comm import test_comm

    if rank:
        faulthandler.dump_traceback_later(120, exit=True, file=sys.stderr)
    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    globals()[fn](rank, ws, torch.device("cuda:0"), test_comm(), *args)
    dist.barrier()
    dist.destroy_process_group()
    if rank:
        faulthandler.cancel_dump_traceback_later()


def test_ws2_rccl(gpu, rccl_env):
    t0 = time.perf_counter()
    cases = [(_mr, ("_case", pdt, state, sgd)) for pdt, state, sgd in CONFIGS]
    cases += [(_mr, ("_case", "bf16", "f32", False, 2, False)),        # two passes, bf16 arena
              (_mr, ("_case", "bf16", "f32", False, 2, True)),         # ... fp32 accumulation arena
              (_mr, ("_case", "bf16", "sr", False, 2, True, False)),   # ... single stream, stochastic
              (_mr, ("_case", "f32", "f32", False, 1, False, True, False, [(1,)])),  # rank 1: nothing
              (_mr, ("_replica",)), (_mr, ("_inf_equals_none",))]
    spawn_batch(2, cases, all_spawned=True)
    print(f"ws=2 ZeRO-3 clipping batch: {time.perf_counter() - t0:.1f} s")
