"""Gradient accumulation in ZeRO-3 update mode (``grad_accumulation=True``): several backward
passes per step(), each reduce-scattered and added to the chunks already held.

Gradients are known exactly (tests/_accum_inputs.py: probe modules whose gradient is a planted
coefficient tensor, integer rank sums), so no GEMM rounding and no ring order enters: after every
backward the accumulated chunks equal the numpy oracle bit for bit, and after every step the
parameters and the optimizer state equal the C oracle applied to those bits with grad_div = ws.
The d16 MLP of tests/test_gpu_zero3.py with every batch fed as two halves stays within 1e-4 of the
reference's ZeRO-2 trajectories.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _accum_inputs as ai
import _sgd_oracle as so
from _zero_run import init_pg, rel, spawn_batch
from conftest import GOLDEN, free_port
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_zero3 import _chunk, _model, _xy

pytestmark = pytest.mark.gpu

LR = 1e-2
SGD = dict(lr=0.05, momentum=0.9)


@pytest.fixture
def pg1():
    init_pg(0, 1, free_port())
    yield
    dist.destroy_process_group()


@pytest.fixture
def rccl_env(monkeypatch):
    monkeypatch.setenv("ZS_TEST_COMM", "rccl")
    monkeypatch.setenv("NCCL_HOSTID", "zs-test-rank0")  # (restored after the test)
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", "lo")
    monkeypatch.setenv("NCCL_IB_DISABLE", "1")
    yield


class Probe(torch.nn.Module):
    """forward() = (weight * c).sum(): the gradient of ``weight`` is ``c`` bit for bit."""

    def __init__(self, w):
        super().__init__()
        self.weight = torch.nn.Parameter(w)
        self.c = None

    def forward(self):
        return (self.weight * self.c).sum()


class ProbeModel(torch.nn.Module):
    def __init__(self, ws):
        super().__init__()
        self.probes = torch.nn.ModuleList(ws)

    def forward(self, on):
        return sum(m() for k, m in enumerate(self.probes) if on[k])


def _host_bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    if t.dtype in (torch.bfloat16, torch.int16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().view(np.uint32).copy()


def _same(got, want, what):
    want = np.ascontiguousarray(want).reshape(-1)
    want = want.view(np.uint32) if want.dtype == np.float32 else want
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first {bad[:4]}: " \
                          f"got {got[bad[:4]]} want {want[bad[:4]]}"


def _rows(a, shape, ws, rank):
    """This rank's dim-0 chunk (torch.chunk rows) of a full-shape array, flat."""
    return np.ascontiguousarray(_chunk(a.reshape(shape), ws, rank)).reshape(-1)


def _init_weights(pdt):
    rng = np.random.default_rng(3)
    out = []
    for s in ai.SHAPES:
        w = (rng.standard_normal(s) * 0.1).astype(np.float32)
        if pdt == "bf16":
            w = zo.bf16_bits_to_f32(zo.f32_to_bf16_bits(w)).reshape(s)
        out.append(w)
    return out


class _Ref:
    """The C (Adam) / numpy (SGD) oracle on full-shape flat arrays; grad_div = ws."""

    def __init__(self, init, pdt, arena, ws, sgd):
        self.pdt, self.arena, self.ws, self.sgd = pdt, arena, ws, sgd
        self.steps = [0] * len(init)
        self.p = [w.reshape(-1).copy() for w in init]           # fp32 params / masters
        if pdt == "bf16":
            self.hi = [zo.f32_to_bf16_bits(w.reshape(-1)) for w in init]
            self.lo = [np.zeros(w.size, np.uint16) for w in init]
        self.m = [np.zeros(w.size, np.float32) for w in init]
        self.v = [np.zeros(w.size, np.float32) for w in init]

    def step(self, i, g):
        """``g``: the accumulated gradient of parameter i in the arena's representation."""
        g = np.ascontiguousarray(g).reshape(-1)
        self.steps[i] += 1
        if self.sgd:
            hp = so.SgdHP(SGD["lr"], SGD["momentum"], first=self.steps[i] == 1, grad_div=float(self.ws))
            assert self.pdt == "f32" and self.arena == "f32"
            self.p[i], self.m[i], _ = so.step_f32(self.p[i], g, None if self.steps[i] == 1 else self.m[i], hp)
            return
        hp = c_oracle.hparams(lr=LR, step=self.steps[i], grad_div=float(self.ws))
        if self.pdt == "bf16":
            c_oracle.adam_bf16_split(self.hi[i], self.lo[i], g, self.m[i], self.v[i], hp)
        elif self.arena == "bf16":  # fp32 parameters, bf16 gradient exchange
            c_oracle.adam_bf16(self.p[i], np.zeros(g.size, np.uint16), g, self.m[i], self.v[i], hp)
        else:
            c_oracle.adam_f32(self.p[i], g, self.m[i], self.v[i], hp)


def _build(dev, pdt, ws, comm, **kw):
    from zero_amd import zero3

    tdt = torch.float32 if pdt == "f32" else torch.bfloat16
    init = _init_weights(pdt)
    model = ProbeModel([Probe(torch.from_numpy(w.copy()).to(dev, tdt)) for w in init])
    params = [m.weight for m in model.probes]
    inner = torch.optim.SGD(params, **SGD) if kw.pop("sgd", False) else torch.optim.Adam(params, lr=LR)
    if comm is not None:
        kw["comm"] = comm
    # ~1-2 KB buckets: a pass launches several
    kw.setdefault("bucket_mb", 2e-3 if pdt == "f32" else 1e-3)
    opt = zero3.ShardedOptimizer(inner, update=True, **kw)
    zero3.register_zero3_hooks(model, opt.param_managers)
    return model, params, opt, init


def _set_coeffs(model, step, pas, rank, arena, dev):
    for k, m in enumerate(model.probes):
        c = torch.from_numpy(ai.coeff(step, pas, rank, k, arena)).to(dev, m.weight.dtype)
        m.c = c


def _schedule(rank, ws, dev, comm, pdt, grad_comm=None, side_stream=True, sgd=False, nsum=None):
    """Three steps of three passes with the skips of tests/_accum_inputs.py.  ``nsum``: the ranks
    whose gradients enter the sums (default all ws; 1 for a simulated job whose other ranks
    contribute zeros)."""
    nsum = nsum or ws
    arena = "bf16" if (pdt == "bf16" or grad_comm) else "f32"
    kw = dict(grad_accumulation=True, side_stream=side_stream, sgd=sgd)
    if grad_comm:
        kw["grad_comm"] = grad_comm
    model, params, opt, init = _build(dev, pdt, ws, comm, **kw)
    red = opt._reducer
    assert red.K >= 2, "the case is meant to launch several buckets per pass"
    ref = _Ref(init, pdt, arena, ws, sgd)
    n = len(params)
    tdt_arena = torch.float32 if arena == "f32" else torch.bfloat16
    launches = 0
    for step in range(ai.STEPS):
        assert opt.accumulated_passes == 0
        before = [(_host_bits(p), {k: _host_bits(v) for k, v in opt._state_views(i).items()})
                  for i, p in enumerate(params)]
        for pas in range(ai.PASSES):
            _set_coeffs(model, step, pas, rank, arena, dev)
            on = [ai.active(step, pas, k) for k in range(n)]
            model(on).backward()  # (no action on p.grad between the passes)
            torch.cuda.synchronize()
            assert opt.accumulated_passes == pas + 1
            if ws > 1 and pas > 0:
                launches += red.K
            assert red.n_accumulate_launches == launches
            assert red.next == red.K
            for i, p in enumerate(params):
                assert p.data.shape == opt._arena.shard_shapes[i]  # back on its shard
                want, had = ai.accumulated(step, pas, i, nsum, arena, arena)
                want = _rows(want, ai.SHAPES[i], ws, rank)
                what = f"rank {rank} step {step} pass {pas} param {i}"
                if ws > 1:
                    s, ln = int(opt._arena.slot[i]), int(opt._arena.ln[i])
                    assert opt.grad_arena().dtype == tdt_arena
                    if had:  # (never reduced this step: the slot keeps the last step's bits)
                        _same(_host_bits(opt.grad_arena()[s:s + ln]), want, what + " (arena)")
                if not had:
                    assert p.grad is None, what
                elif ws == 1 or not grad_comm:
                    assert p.grad.shape == p.shape and p.grad.dtype == p.dtype
                    _same(_host_bits(p.grad), want, what + " (p.grad)")
        calls = list(getattr(opt.comm, "calls", []))
        opt.step()
        torch.cuda.synchronize()
        # nothing is reduced again: every bucket of every pass went out in its backward.  (step()
        # ends with the runtime's prefetch of the next iteration's first all-gather, as it always
        # has, so gathers — and only gathers — may join the communicator's log here.)
        new = list(getattr(opt.comm, "calls", []))[len(calls):]
        assert all(c[0] in ("ag", "ag_group") for c in new), new
        assert red.n_accumulate_launches == launches and opt.accumulated_passes == 0
        assert all(p.grad is None for p in params)
        for i, p in enumerate(params):
            g, had = ai.accumulated(step, ai.PASSES - 1, i, nsum, arena, arena)
            what = f"rank {rank} after step {step} param {i}"
            if not had:  # skipped for the whole step: nothing of it moves
                assert (i, step) == ai.SKIP_IN_STEP
                _same(_host_bits(p), before[i][0], what + " moved")
                for k, v in opt._state_views(i).items():
                    _same(_host_bits(v), before[i][1][k], what + f" {k} moved")
                assert ref.steps[i] == step and int(opt._steps[i]) == (step if p.numel() else 0)
                continue
            ref.step(i, g)
            if p.numel() == 0:  # (this rank owns no row of it: nothing to update or count)
                continue
            assert int(opt._steps[i]) == ref.steps[i]
            shp = ai.SHAPES[i]
            if pdt == "bf16":
                _same(_host_bits(p), _rows(ref.hi[i], shp, ws, rank), what)
                _same(_host_bits(opt._state_views(i)["master_residual"]),
                      _rows(ref.lo[i], shp, ws, rank), what + " residual")
            else:
                _same(_host_bits(p), _rows(ref.p[i], shp, ws, rank), what)
            st = opt.optimizer.state[p]
            if sgd:
                _same(_host_bits(st["momentum_buffer"]), _rows(ref.m[i], shp, ws, rank), what + " buffer")
            else:
                assert int(st["step"].item()) == ref.steps[i]
                _same(_host_bits(st["exp_avg"]), _rows(ref.m[i], shp, ws, rank), what + " exp_avg")
                _same(_host_bits(st["exp_avg_sq"]), _rows(ref.v[i], shp, ws, rank), what + " exp_avg_sq")
    if ws > 1:  # the staging buffer: the largest bucket's range, bucket / ws of gradient plus pads
        stg = opt.grad_staging()
        es = params[0].element_size()
        bucket_bytes = int((2e-3 if pdt == "f32" else 1e-3) * (1 << 20))
        bound = 0
        for g in red.groups:
            full = sum(int(np.prod(ai.SHAPES[i])) for i in g)
            assert full * es <= bucket_bytes or len(g) == 1
            # a chunk is at most 1 / ws of its parameter plus one row; a pad is under 64 elements
            rows = sum(int(np.prod(ai.SHAPES[i][1:])) for i in g)
            bound = max(bound, full // ws + rows + 63 * len(g))
        assert stg is not None and stg.dtype == tdt_arena
        assert stg.numel() == max(ln for _, ln in red._range) and 0 < stg.numel() <= bound
    else:
        assert opt.grad_staging() is None and red.n_accumulate_launches == 0
    return opt


# ---- the inputs themselves (CPU arithmetic, asserted where the GPU cases run) -------------------
@pytest.mark.parametrize("arena", ["f32", "bf16"])
def test_inputs_make_accumulation_inexact(arena):
    for ws in (1, 2, 3):
        total, inexact, ties = ai.addition_stats(ws, arena, arena)
        print(f"ws={ws} {arena}: {total} additions, {inexact} inexact, {ties} ties")
        assert total > 3000 and 4 * inexact >= total and ties > 0


def test_probe_gradient_is_the_coefficient(gpu):
    for dt in (torch.float32, torch.bfloat16):
        arena = "f32" if dt == torch.float32 else "bf16"
        for pas in range(ai.PASSES):
            c = torch.from_numpy(ai.coeff(0, pas, 1, 4, arena)).to(gpu, dt)
            m = Probe(torch.randn(ai.SHAPES[4], device=gpu).to(dt))
            m.c = c
            m().backward()
            assert torch.equal(m.weight.grad, c)


# ---- ws = 1 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdt", ["f32", "bf16"])
def test_ws1_schedule(gpu, pg1, pdt):
    _schedule(0, 1, gpu, None, pdt)


# ---- rank 0 of a simulated ws = 3 job: an asynchronous per-parameter communicator ---------------
@pytest.fixture
def sim3(pg1, monkeypatch):
    import zero_amd.zero3 as z3

    real_get = z3.get
    monkeypatch.setattr(z3, "get", lambda what, dm=None: {"ws": 3, "rank": 0}[what]
                        if what in ("ws", "rank") else real_get(what, dm))
    yield


@pytest.mark.parametrize("side_stream", [True, False], ids=["side", "single"])
@pytest.mark.parametrize("pdt", ["f32", "bf16"])
def test_simulated_rank_schedule(gpu, sim3, pdt, side_stream):
    """SimRankComm has no table form and never synchronises with the host: every bucket takes the
    per-parameter reduce path, its device copies ordered by the streams alone — the staging
    buffer's zero fill included, which must be behind the first accumulating reduce-scatter."""
    from _gloo_comm import SimRankComm

    opt = _schedule(0, 3, gpu, SimRankComm(3, 0), pdt, None, side_stream, nsum=1)
    assert not opt._reducer._rs_tables and all(rf is None for rf in opt._reducer._rfast.values())


def test_memory_report_counts_the_staging_buffer(gpu, sim3):
    from _gloo_comm import SimRankComm
    from zero_amd.training_utils.memory import memory_report

    model, params, opt, _ = _build(gpu, "bf16", 3, SimRankComm(3, 0), grad_accumulation=True)
    on = [True] * len(params)
    _set_coeffs(model, 0, 0, 0, "bf16", gpu)
    model(on).backward()
    assert opt.grad_staging() is None
    first = memory_report(model, opt, gpu)
    _set_coeffs(model, 0, 1, 0, "bf16", gpu)
    model(on).backward()
    second = memory_report(model, opt, gpu)
    stg = opt.grad_staging()
    assert stg is not None and stg.numel() > 0
    mib = stg.numel() * stg.element_size() / float(1 << 20)
    assert abs((second.grads_mb - first.grads_mb) - mib) < 1e-9
    assert abs((second.grads_physical_mb - first.grads_physical_mb)
               - stg.untyped_storage().nbytes() / float(1 << 20)) < 1e-9
    opt.step()


# ---- ws = 2, 3: the gloo-staged communicator -----------------------------------------------------
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


SCHEDULE_CASES = [(pdt, gc, side) for pdt, gc in (("f32", None), ("bf16", None), ("f32", "bf16"))
                  for side in (True, False)]


def _semantics(rank, ws, dev, comm):
    """One backward per step is the flag off, bit for bit; zero_grad() discards; step() right
    after the passes launches no collective."""
    from zero_amd import zero3

    runs = []
    for flag in (False, True):
        model, params, opt, _ = _build(dev, "bf16", ws, comm, grad_accumulation=flag)
        for step in range(5):
            _set_coeffs(model, step % ai.STEPS, step % ai.PASSES, rank, "bf16", dev)
            model([True] * len(params)).backward()
            opt.step()
            opt.zero_grad()
        torch.cuda.synchronize()
        runs.append([_host_bits(p) for p in params] + [_host_bits(opt._state)])
        if flag:
            assert opt._reducer.n_accumulate_launches == 0 and opt.grad_staging() is None
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    # backward, zero_grad(), backward, step() equals one backward
    outs = []
    for twice in (False, True):
        model, params, opt, _ = _build(dev, "f32", ws, comm, grad_accumulation=True)
        if twice:
            _set_coeffs(model, 0, 0, rank, "f32", dev)
            model([True] * len(params)).backward()
            assert opt.accumulated_passes == 1
            opt.zero_grad()
            assert opt.accumulated_passes == 0 and all(p.grad is None for p in params)
        _set_coeffs(model, 1, 0, rank, "f32", dev)
        model([True] * len(params)).backward()
        assert opt.accumulated_passes == 1
        opt.step()
        torch.cuda.synchronize()
        assert opt._reducer.n_accumulate_launches == 0
        outs.append([_host_bits(p) for p in params])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="update mode"):
        zero3.ShardedOptimizer(torch.optim.Adam([torch.nn.Parameter(torch.zeros(4, device=dev))]),
                               grad_accumulation=True)


def _fixture_halves(rank, ws, dev, comm):
    """The d16 MLP on the reference's ZeRO-2 trajectory, every rank's batch as two halves."""
    from zero_amd import zero3

    z = np.load(GOLDEN / f"traj_z2_ws{ws}_d16_distinct.npz")
    model = _model(z, dev)
    opt = zero3.ShardedOptimizer(torch.optim.Adam(model.parameters(), lr=1e-3), update=True,
                                 comm=comm, bucket_mb=2e-3, grad_accumulation=True)
    zero3.register_zero3_hooks(model, opt.param_managers)
    params = list(model.parameters())
    x, y = _xy(z, rank, dev)
    h = x.shape[0] // 2
    assert x.shape[0] == 16 and int(z["steps"]) == 10
    for t in range(10):
        opt.zero_grad()
        for xs, ys in ((x[:h], y[:h]), (x[h:], y[h:])):
            (torch.nn.functional.mse_loss(model(xs), ys) / 2).backward()
        assert opt.accumulated_passes == 2
        opt.step()
        for i, p in enumerate(params):
            want = _chunk(z[f"r{rank}_t{t}_p{i}"], ws, rank)
            assert rel(p.detach().cpu().numpy(), want) <= 1e-4, (t, i)
    assert opt._reducer.n_accumulate_launches == 10 * opt._reducer.K


def _raising_backward(rank, ws, dev, comm):
    """A backward that raises inside an accumulating pass: step() refuses until zero_grad()."""
    model, params, opt, _ = _build(dev, "f32", ws, comm, grad_accumulation=True)
    _set_coeffs(model, 0, 0, rank, "f32", dev)
    model([True] * len(params)).backward()

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            raise ValueError("boom")

    _set_coeffs(model, 0, 1, rank, "f32", dev)
    on = [True] * len(params)
    # (the failing branch is built first, so autograd reaches it after the other branch's
    # gradients have been accumulated and counted)
    boom = Boom.apply(sum(m() for m in model.probes[:3]))
    loss = sum(m() for m in model.probes[3:]) + boom
    with pytest.raises(ValueError, match="boom"):
        loss.backward()
    with pytest.raises(RuntimeError, match="did not finish"):
        opt.step()
    opt.zero_grad()
    assert opt.accumulated_passes == 0
    ref_model, ref_params, ref_opt, _ = _build(dev, "f32", ws, comm, grad_accumulation=True)
    for m, o in ((model, opt), (ref_model, ref_opt)):
        _set_coeffs(m, 1, 0, rank, "f32", dev)
        m(on).backward()
        o.step()
    torch.cuda.synchronize()
    for p, q in zip(params, ref_params):
        assert np.array_equal(_host_bits(p), _host_bits(q))


@pytest.mark.parametrize("ws", [2, 3])
def test_multirank_schedule(gpu, ws):
    cases = [(_mr, ("_schedule", pdt, gc, side)) for pdt, gc, side in SCHEDULE_CASES]
    cases.append((_mr, ("_schedule", "f32", None, True, True)))  # SGD with momentum
    spawn_batch(ws, cases)


@pytest.mark.parametrize("ws", [2, 3])
def test_multirank_semantics_and_fixture(gpu, ws):
    spawn_batch(ws, [(_mr, ("_semantics",)), (_mr, ("_fixture_halves",)),
                     (_mr, ("_raising_backward",))])


def test_ws2_real_rccl(gpu, rccl_env):
    """bf16 with the split master through the product communicator and the side stream: the
    one-call ReduceFast path, its second instance bound to the staging addresses."""
    spawn_batch(2, [(_mr, ("_schedule_rccl",))], all_spawned=True)


def _schedule_rccl(rank, ws, dev, comm):
    from zero_amd import zero3

    opt = _schedule(rank, ws, dev, comm, "bf16", None, True)
    assert zero3._hostext is not None and hasattr(comm, "reduce_scatter_group_synced_raw")
    # buckets of even chunks went out through ReduceFast in both kinds of pass (the (16, 16)
    # bucket here; uneven chunks take the general path's synced group)
    rfs = opt._reducer._rfast
    assert {acc for (_, acc) in rfs} == {False, True}
    for k, g in enumerate(opt._reducer.groups):
        even = all(ai.SHAPES[i][0] % ws == 0 for i in g)
        assert (rfs[(k, False)] is not None) == (rfs[(k, True)] is not None) == even
    assert any(rf is not None for rf in rfs.values())
