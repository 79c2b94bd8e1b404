"""``accumulation_dtype=torch.float32`` in ZeRO-3 update mode: from a step's second backward on,
the bf16 gradient chunks are summed in an fp32 arena (zs_accumulate_widen) and step() reads that
arena through the fp32-gradient instances of the fused update.

Built on the fixtures and worker machinery of tests/test_gpu_zero3_accumulate.py (gloo-staged ranks,
``SimRankComm``, one real-RCCL case at ws = 2) with its way of knowing every pass's chunks exactly:
probe modules whose gradient is a planted coefficient tensor, integers in [-42, 42] times a
per-pass power of two, so every rank sum is exact in bf16 under any reduction order.  The probes
have the parameter shapes of a bf16 MLP, Linear(96, 80) and Linear(80, 33) with their biases: uneven
dim-0 chunks at ws = 2 (33 rows) and ws = 3 (80 rows) and alignment pads behind the biases.  The
passes' scales (1, 2^-9, 2^-19, 2^-27) make the fp32 sum inexact from the third pass on and make
the bf16 sum lose every later pass.

After every multi-pass backward the fp32 arena's slots equal the numpy restatement
(tests/_accum32_oracle.py) of the passes' delivered chunks, in pass order; after every step the
parameters, the residual and the optimizer state equal the composed oracle on that sum with
grad_div = ws, bit for bit.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _accum32_oracle as a32
import _sgd_oracle as so
from _zero_run import init_pg, spawn_batch
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_zero3_accumulate import (Probe, ProbeModel, _host_bits, _rows, _same,  # noqa: F401
                                       pg1, rccl_env, sim3)

pytestmark = pytest.mark.gpu

SHAPES = [(80, 96), (80,), (33, 80), (33,)]
SCALES = (1.0, 2.0 ** -9, 2.0 ** -19, 2.0 ** -27)
LR = 1e-2
SGD = dict(lr=0.05, momentum=0.9)
BUCKET_MB = 8e-3  # two buckets of bf16 gradient, four of fp32
SKIP = (1, 1)     # (module, pass): no gradient in the second pass of any step


def active(pas, mod):
    return (mod, pas) != SKIP


def coeff_ints(step, pas, rank, mod):
    n = int(np.prod(SHAPES[mod]))
    e = np.arange(n, dtype=np.uint64)
    h = (e * np.uint64(2654435761) + np.uint64(40503 * (step + 1) + 9176 * (pas + 1)
                                                 + 65599 * (rank + 1) + 31337 * (mod + 1)))
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(13))) % np.uint64(85)
    return h.astype(np.int64) - 42


def coeff(step, pas, rank, mod):
    return (coeff_ints(step, pas, rank, mod) * SCALES[pas]).astype(np.float32).reshape(SHAPES[mod])


def delivered(step, pas, mod, nsum):
    """The bf16 chunk values pass ``pas`` delivers for module ``mod`` (full shape, uint16 bits): the
    exact sum over the contributing ranks, zeros when the module has no gradient in that pass."""
    if not active(pas, mod):
        return np.zeros(int(np.prod(SHAPES[mod])), np.uint16)
    s = sum(coeff_ints(step, pas, r, mod) for r in range(nsum))
    assert np.abs(s).max() <= 126
    x = (s * SCALES[pas]).astype(np.float32)
    bits = zo.f32_to_bf16_bits(x)
    assert np.array_equal(zo.bf16_bits_to_f32(bits), x), "a rank sum is not exact in bf16"
    return bits


def test_inputs_make_both_sums_inexact():
    """The bf16 running sum loses the later passes and the fp32 one rounds from the third pass on."""
    chunks = [delivered(0, p, 0, 3) for p in range(4)]
    exact = a32.exact_sum(chunks)
    s3 = a32.accumulate_passes(chunks[:3]).astype(np.float64)
    assert (s3 != a32.exact_sum(chunks[:3])).mean() > 0.1
    assert (np.abs(a32.accumulate_passes(chunks).astype(np.float64) - exact)
            <= a32.fp32_bound(chunks)).all()
    bf = chunks[0]
    for c in chunks[1:]:
        bf = zo.f32_to_bf16_bits(zo.bf16_bits_to_f32(bf) + zo.bf16_bits_to_f32(c))
    live = exact != 0
    assert (np.abs(zo.bf16_bits_to_f32(bf).astype(np.float64) - exact)[live]
            > a32.fp32_bound(chunks)[live]).mean() > 0.9


def _init_weights(pdt):
    rng = np.random.default_rng(7)
    out = []
    for s in SHAPES:
        w = (rng.standard_normal(s) * 0.1).astype(np.float32)
        if pdt == "bf16":
            w = zo.bf16_bits_to_f32(zo.f32_to_bf16_bits(w)).reshape(s)
        out.append(w)
    return out


def _build(dev, pdt, comm, **kw):
    from zero_amd import zero3

    tdt = torch.float32 if pdt == "f32" else torch.bfloat16
    init = _init_weights(pdt)
    model = ProbeModel([Probe(torch.from_numpy(w.copy()).to(dev, tdt)) for w in init])
    params = [m.weight for m in model.probes]
    inner = torch.optim.SGD(params, **SGD) if kw.pop("sgd", False) else torch.optim.Adam(params, lr=LR)
    if comm is not None:
        kw["comm"] = comm
    kw.setdefault("bucket_mb", BUCKET_MB)
    kw.setdefault("grad_accumulation", True)
    opt = zero3.ShardedOptimizer(inner, update=True, **kw)
    zero3.register_zero3_hooks(model, opt.param_managers)
    return model, params, opt, init


def _set_coeffs(model, step, pas, rank, dev):
    for k, m in enumerate(model.probes):
        m.c = torch.from_numpy(coeff(step, pas, rank, k)).to(dev, m.weight.dtype)


def _backward(model, step, pas, rank, dev):
    _set_coeffs(model, step, pas, rank, dev)
    model([active(pas, k) for k in range(len(SHAPES))]).backward()


class _Ref:
    """The composed oracle on full-shape flat arrays; grad_div = ws."""

    def __init__(self, init, pdt, ws, sgd):
        self.pdt, self.ws, self.sgd = pdt, ws, sgd
        self.steps = [0] * len(init)
        self.p = [w.reshape(-1).copy() for w in init]
        self.hi = [zo.f32_to_bf16_bits(w.reshape(-1)) for w in init]
        self.lo = [np.zeros(w.size, np.uint16) for w in init]
        self.m = [np.zeros(w.size, np.float32) for w in init]
        self.v = [np.zeros(w.size, np.float32) for w in init]

    def step(self, i, acc):
        """``acc``: the arena's content for parameter i: bf16 bits (one pass) or the fp32 sum."""
        self.steps[i] += 1
        wide = acc.dtype == np.float32
        if self.sgd:
            assert self.pdt == "bf16"
            hp = so.SgdHP(SGD["lr"], SGD["momentum"], first=self.steps[i] == 1, grad_div=float(self.ws))
            buf = None if self.steps[i] == 1 else self.m[i]
            if wide:
                self.hi[i], self.lo[i], self.m[i] = a32.sgd_f32grad_split(self.hi[i], self.lo[i], acc, buf, hp)
            else:
                self.hi[i], self.lo[i], self.m[i], _ = so.step_split(self.hi[i], self.lo[i], acc, buf, hp)
            return
        hp = c_oracle.hparams(lr=LR, step=self.steps[i], grad_div=float(self.ws))
        if self.pdt == "bf16":
            if wide:
                a32.adam_f32grad_split(self.hi[i], self.lo[i], acc, self.m[i], self.v[i], hp)
            else:
                c_oracle.adam_bf16_split(self.hi[i], self.lo[i], acc, self.m[i], self.v[i], hp)
        elif wide:  # fp32 parameters, bf16 exchange, fp32 sum: the existing fp32 instances
            c_oracle.adam_f32(self.p[i], acc, self.m[i], self.v[i], hp)
        else:
            c_oracle.adam_bf16(self.p[i], np.zeros(acc.size, np.uint16), acc, self.m[i], self.v[i], hp)


def _check_state(opt, params, ref, pdt, sgd, ws, rank, what):
    for i, p in enumerate(params):
        if p.numel() == 0:
            continue
        shp, w = SHAPES[i], f"{what} param {i}"
        assert int(opt._steps[i]) == ref.steps[i]
        if pdt == "bf16":
            _same(_host_bits(p), _rows(ref.hi[i], shp, ws, rank), w)
            _same(_host_bits(opt._state_views(i)["master_residual"]), _rows(ref.lo[i], shp, ws, rank),
                  w + " residual")
        else:
            _same(_host_bits(p), _rows(ref.p[i], shp, ws, rank), w)
        st = opt.optimizer.state[p]
        if sgd:
            _same(_host_bits(st["momentum_buffer"]), _rows(ref.m[i], shp, ws, rank), w + " buffer")
        else:
            _same(_host_bits(st["exp_avg"]), _rows(ref.m[i], shp, ws, rank), w + " exp_avg")
            _same(_host_bits(st["exp_avg_sq"]), _rows(ref.v[i], shp, ws, rank), w + " exp_avg_sq")


def _schedule(rank, ws, dev, comm, passes, pdt="bf16", grad_comm=None, side_stream=True, sgd=False,
              nsum=None):
    """One step per entry of ``passes`` (backward passes in that step)."""
    nsum = nsum or ws
    kw = dict(accumulation_dtype=torch.float32, side_stream=side_stream, sgd=sgd)
    if grad_comm:
        kw["grad_comm"] = grad_comm
    model, params, opt, init = _build(dev, pdt, comm, **kw)
    red = opt._reducer
    assert red.K >= 2 and red.widen and opt._acc_widen
    ref = _Ref(init, pdt, ws, sgd)
    widen = 0
    seen_multi = False
    for step, npass in enumerate(passes):
        chunks = [[] for _ in SHAPES]
        for pas in range(npass):
            if not seen_multi and pas == 0:
                assert opt._A is None and opt.accumulation_arena() is None  # nothing allocated yet
            _backward(model, step, pas, rank, dev)
            torch.cuda.synchronize()
            assert opt.accumulated_passes == pas + 1
            if pas:
                widen += red.K
                seen_multi = True
            assert red.n_widen_launches == widen and red.n_accumulate_launches == 0
            arena = opt.grad_arena()
            if pas == 0:
                assert arena is opt._G and arena.dtype == torch.bfloat16
                assert opt.accumulation_arena_dtype == torch.bfloat16
            else:
                assert arena is opt._A and arena.dtype == torch.float32
                assert opt.accumulation_arena_dtype == torch.float32
                assert arena.numel() == opt._G.numel() and opt.accumulation_arena() is arena
            for i, p in enumerate(params):
                chunks[i].append(delivered(step, pas, i, nsum))
                want = _rows(a32.accumulate_passes(chunks[i]), SHAPES[i], ws, rank)
                s, ln = int(opt._arena.slot[i]), int(opt._arena.ln[i])
                what = f"rank {rank} step {step} pass {pas} param {i}"
                _same(_host_bits(arena[s:s + ln]), want, what + " (arena)")
                if pas or grad_comm:
                    assert p.grad is None, what  # an fp32 sum cannot be a bf16 parameter's .grad
                else:
                    assert p.grad.dtype == p.dtype and p.grad.shape == p.shape
                    _same(_host_bits(p.grad), want, what + " (p.grad)")
        opt.step()
        torch.cuda.synchronize()
        assert red.n_widen_launches == widen and opt.accumulated_passes == 0
        assert opt.grad_arena() is opt._G and all(p.grad is None for p in params)
        for i in range(len(params)):
            ref.step(i, a32.accumulate_passes(chunks[i]))
        _check_state(opt, params, ref, pdt, sgd, ws, rank, f"rank {rank} after step {step}")
    # one set per arena, built once each: alternating steps neither rebuild nor run a stale set
    arenas = {ck[3] for ck in opt._adam_cache}
    assert arenas == {n > 1 for n in passes} and len(opt._adam_cache) == len(arenas)
    assert not opt._retired
    assert set(opt._fast_sets) == arenas
    return opt


def _one_pass_is_untouched(rank, ws, dev, comm):
    """One backward per step: nothing allocated, no widen launch, and parameters and state
    bit-identical to the option off."""
    runs = []
    for dt in (None, torch.float32):
        model, params, opt, _ = _build(dev, "bf16", comm, accumulation_dtype=dt)
        for step in range(3):
            _backward(model, step, step, rank, dev)
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        red = opt._reducer
        assert red.n_widen_launches == 0 and red.n_accumulate_launches == 0
        assert opt._A is None and opt.grad_staging() is None
        assert opt.grad_arena() is opt._G and opt.accumulation_arena_dtype == torch.bfloat16
        assert all(ck[3] is False for ck in opt._adam_cache)
        runs.append([_host_bits(p) for p in params] + [_host_bits(opt._state)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def _fp32_chunks_are_untouched(rank, ws, dev, comm):
    """fp32 parameters without grad_comm: the arena already is fp32; the option changes nothing."""
    runs = []
    for dt in (None, torch.float32):
        model, params, opt, _ = _build(dev, "f32", comm, accumulation_dtype=dt)
        assert not opt._acc_widen and not opt._reducer.widen
        for step in range(2):
            for pas in range(3):
                _backward(model, step, pas, rank, dev)
                assert opt.accumulation_arena_dtype == torch.float32 and opt.grad_arena() is opt._G
            opt.step()
        torch.cuda.synchronize()
        assert opt._reducer.n_widen_launches == 0 and opt._A is None
        assert opt._reducer.n_accumulate_launches == 2 * 2 * opt._reducer.K
        runs.append([_host_bits(p) for p in params] + [_host_bits(opt._state)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def _planted(rank, ws, dev, comm):
    """1.0, then 2^-9 seven times, through the real path: the fp32 arena holds 1 + 7 * 2^-9 where
    the bf16 one stays at 1.0 (every add a tie to even)."""
    got = {}
    for dt in (None, torch.float32):
        model, params, opt, _ = _build(dev, "bf16", comm, accumulation_dtype=dt)
        on = [True] * len(params)
        for pas, x in enumerate(a32.PLANTED):
            for k, m in enumerate(model.probes):  # rank 0 alone contributes: the rank sum is x
                m.c = torch.full(SHAPES[k], x if rank == 0 else 0.0, device=dev,
                                 dtype=m.weight.dtype)
            model(on).backward()
        torch.cuda.synchronize()
        assert opt.accumulated_passes == len(a32.PLANTED)
        arena = opt.grad_arena()
        s, ln = int(opt._arena.slot[0]), int(opt._arena.ln[0])
        got[dt] = arena[s:s + ln].float().cpu().numpy().astype(np.float64)
        assert arena.dtype == (torch.bfloat16 if dt is None else torch.float32)
        opt.step()
    exact = 1.0 + 7 * 2.0 ** -9
    assert got[None].size and (got[None] == 1.0).all()
    assert (got[torch.float32] == exact).all()
    bound = a32.fp32_bound(a32.planted_bits())[0]
    assert abs(1.0 - exact) > 1e4 * bound


def _zero_grad_and_raising(rank, ws, dev, comm):
    """zero_grad() between passes discards the accumulation; a raising backward makes step() raise
    until zero_grad()."""
    model, params, opt, _ = _build(dev, "bf16", comm, accumulation_dtype=torch.float32)
    ref_model, ref_params, ref_opt, _ = _build(dev, "bf16", comm, accumulation_dtype=torch.float32)
    _backward(model, 0, 0, rank, dev)
    _backward(model, 0, 1, rank, dev)
    assert opt.accumulated_passes == 2 and opt.grad_arena() is opt._A
    opt.zero_grad()
    assert opt.accumulated_passes == 0 and opt.grad_arena() is opt._G
    assert all(p.grad is None for p in params)
    for m, o in ((model, opt), (ref_model, ref_opt)):
        _backward(m, 1, 0, rank, dev)
        o.step()
    torch.cuda.synchronize()
    assert ref_opt._A is None and opt._A is not None
    for p, q in zip(params, ref_params):
        assert np.array_equal(_host_bits(p), _host_bits(q))

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            raise ValueError("boom")

    _backward(model, 2, 0, rank, dev)
    _set_coeffs(model, 2, 2, rank, dev)
    boom = Boom.apply(sum(m() for m in model.probes[:2]))
    loss = sum(m() for m in model.probes[2:]) + boom
    with pytest.raises(ValueError, match="boom"):
        loss.backward()
    with pytest.raises(RuntimeError, match="did not finish"):
        opt.step()
    opt.zero_grad()
    assert opt.accumulated_passes == 0 and opt.grad_arena() is opt._G
    for m, o in ((model, opt), (ref_model, ref_opt)):
        _backward(m, 2, 0, rank, dev)
        _backward(m, 2, 1, rank, dev)
        o.step()
    torch.cuda.synchronize()
    for p, q in zip(params, ref_params):
        assert np.array_equal(_host_bits(p), _host_bits(q))
    assert np.array_equal(_host_bits(opt._state), _host_bits(ref_opt._state))


# ---- ws = 1: no arena, the option changes nothing ----------------------------------------------
def test_ws1_option_changes_nothing(gpu, pg1):
    runs = []
    for dt in (None, torch.float32):
        model, params, opt, _ = _build(gpu, "bf16", None, accumulation_dtype=dt)
        for step in range(2):
            for pas in range(3):
                _backward(model, step, pas, 0, gpu)
            assert opt.grad_arena() is None and opt.accumulation_arena_dtype is None
            opt.step()
        torch.cuda.synchronize()
        assert opt._A is None and opt._reducer.n_widen_launches == 0
        runs.append([_host_bits(p) for p in params] + [_host_bits(opt._state)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- rank 0 of a simulated ws = 3 job ----------------------------------------------------------
@pytest.mark.parametrize("side_stream", [True, False], ids=["side", "single"])
def test_simulated_rank_schedule(gpu, sim3, side_stream):
    """SimRankComm never synchronises with the host: the fp32 arena's zero fill and every widen
    launch are ordered by the streams alone."""
    from _gloo_comm import SimRankComm

    _schedule(0, 3, gpu, SimRankComm(3, 0), (1, 3, 1, 4), side_stream=side_stream, nsum=1)


def test_simulated_rank_semantics(gpu, sim3):
    from _gloo_comm import SimRankComm

    _one_pass_is_untouched(0, 3, gpu, SimRankComm(3, 0))
    _fp32_chunks_are_untouched(0, 3, gpu, SimRankComm(3, 0))


def test_memory_report_counts_the_accumulation_arena(gpu, sim3):
    from _gloo_comm import SimRankComm
    from zero_amd.training_utils.memory import memory_report

    model, params, opt, _ = _build(gpu, "bf16", SimRankComm(3, 0), accumulation_dtype=torch.float32)
    _backward(model, 0, 0, 0, gpu)
    first = memory_report(model, opt, gpu)
    _backward(model, 0, 1, 0, gpu)
    second = memory_report(model, opt, gpu)
    A, stg = opt.accumulation_arena(), opt.grad_staging()
    assert A is not None and A.dtype == torch.float32 and A.numel() == opt._G.numel()
    # the chunk views came off the parameters at the second forward's gather: count them back
    views = sum(int(opt._arena.ln[i]) for i in range(len(params))) * 2
    mib = (A.numel() * 4 + stg.numel() * 2 - views) / float(1 << 20)
    assert abs((second.grads_mb - first.grads_mb) - mib) < 1e-9
    opt.step()


# ---- ws = 2, 3: the gloo-staged communicator ---------------------------------------------------
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


@pytest.mark.parametrize("ws", [2, 3])
def test_multirank_schedules(gpu, ws):
    spawn_batch(ws, [(_mr, ("_schedule", (1, 2, 1))),
                     (_mr, ("_schedule", (3, 1, 4), "bf16", None, False)),
                     (_mr, ("_schedule", (2, 1, 3), "f32", "bf16")),       # grad_comm over fp32 params
                     (_mr, ("_schedule", (1, 3, 2), "bf16", None, True, True))])  # SGD with momentum


@pytest.mark.parametrize("ws", [2, 3])
def test_multirank_semantics(gpu, ws):
    spawn_batch(ws, [(_mr, ("_one_pass_is_untouched",)), (_mr, ("_planted",)),
                     (_mr, ("_zero_grad_and_raising",))])


def test_ws2_real_rccl(gpu, rccl_env):
    """The product communicator and the side stream: the one-call ReduceFast path of both kinds of
    pass, followed by the widen launch."""
    spawn_batch(2, [(_mr, ("_schedule", (2, 1, 4)))], all_spawned=True)
