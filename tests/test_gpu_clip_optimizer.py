"""``ShardedOptimizer(..., max_grad_norm=...)``: global gradient-norm clipping inside ``step()``.

Adam's update is nearly invariant to the gradient's scale, so parameters alone cannot show that
clipping happened: every trajectory below compares exp_avg and exp_avg_sq too, and runs 3 steps
whose gradients are scaled x1, x40 and x0.05 with ``max_grad_norm`` four times the first step's
norm, so the coefficients are exactly 1, about 0.1 and exactly 1 again.

fp32 cases follow a CPU replica (``clip_grad_norm_`` + ``torch.optim.AdamW``) to 1e-6 relative, the
bound of the existing workers; bf16 split-master cases equal the C oracle bit for bit, fed the
pre-clipped gradient with the coefficient the device reported (tests/test_gpu_gradnorm.py
``_ref_step``, pinned there on the CPU).
"""
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist

from conftest import free_port
from _zero_run import init_pg, rel, set_grad, spawn_batch
from oracle import zero_oracle as zo
from test_gpu_gradnorm import _bits, _ref_init, _ref_step

pytestmark = pytest.mark.gpu

SCALES = (1.0, 40.0, 0.05)
ONE = 0x3F800000


@pytest.fixture
def pg1():
    own = not dist.is_initialized()
    if own:
        init_pg(0, 1, free_port())
    yield
    if own:
        dist.destroy_process_group()


@pytest.fixture
def rccl_env(monkeypatch):
    monkeypatch.setenv("ZS_TEST_COMM", "rccl")
    monkeypatch.setenv("NCCL_HOSTID", "zs-test-rank0")  # (restored after the test)
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", "lo")
    monkeypatch.setenv("NCCL_IB_DISABLE", "1")
    yield


def _f32(t):
    return np.float32(t.item())


def _norm64(grads):
    return float(np.sqrt(sum(np.sum(np.asarray(g, np.float64) ** 2) for g in grads if g is not None)))


class _Replica:
    """The reference on the CPU: clip_grad_norm_ then torch's AdamW, on the averaged gradients."""

    def __init__(self, init, groups):
        self.params = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
        self.opt = torch.optim.AdamW([dict(params=[self.params[i] for i in idx], **kw)
                                      for idx, kw in groups])

    def step(self, grads, max_norm):
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else torch.from_numpy(np.ascontiguousarray(g))
        norm = torch.nn.utils.clip_grad_norm_(self.params, max_norm)
        self.opt.step()
        return float(norm)

    def state(self, i, name):
        return self.opt.state[self.params[i]][name].numpy()


def _compare_fp32(opt, params, rep, owned, tol=1e-6):
    for i, p in enumerate(params):
        if p.numel() == 0:
            continue
        assert rel(p.detach().cpu().numpy(), rep.params[i].detach().numpy()) <= tol, f"param {i}"
        if i in owned:
            st = opt.optimizer.state[p]
            for name in ("exp_avg", "exp_avg_sq"):
                assert rel(st[name].cpu().numpy(), rep.state(i, name)) <= tol, f"{name} {i}"


def _grads(rng, shapes, scale):
    return [(rng.standard_normal(s) * 1e-2 * scale).astype(np.float32) for s in shapes]


# ---------------------------------------------------------------------------------------------
# world size 1
# ---------------------------------------------------------------------------------------------
def test_ws1_fp32_two_groups(gpu, pg1):
    """Injected gradients, two AdamW groups, a 0-size parameter, and one parameter without a
    gradient in step 2 (the general partitioning path; torch leaves it out of the norm)."""
    from zero_amd import zero2

    shapes = [(136, 64), (48,), (0,), (7, 5), (64, 3)]
    groups = [([0, 1, 2], dict(lr=1e-3, weight_decay=1e-2)), ([3, 4], dict(lr=2e-3, weight_decay=0.0))]
    rng = np.random.default_rng(3)
    init = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    steps = [_grads(rng, shapes, s) for s in SCALES]
    steps[1][3] = None
    max_norm = 4.0 * _norm64(steps[0])
    rep = _Replica(init, groups)
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(gpu)) for a in init]
    opt = zero2.ShardedOptimizer(
        torch.optim.AdamW([dict(params=[params[i] for i in idx], **kw) for idx, kw in groups]),
        max_grad_norm=max_norm)
    coefs = []
    for grads in steps:
        opt.zero_grad()
        for p, g in zip(params, grads):
            if g is not None:
                p.grad = torch.from_numpy(g).to(gpu)
        opt.step()
        want = rep.step(grads, max_norm)
        got = float(opt.last_grad_norm.item())
        print(f"norm {got!r} vs torch {want!r}, coef {opt.last_clip_coef.item()!r}")
        assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.dtype == torch.float32
        assert abs(got - want) <= 1e-6 * want
        coefs.append(_f32(opt.last_clip_coef))
        assert opt.last_norm_bytes == 4 * sum(g.size for g in grads if g is not None)
        _compare_fp32(opt, params, rep, owned=range(len(params)))
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE
    assert 0.05 < coefs[1] < 0.2


def test_ws1_bf16_split_through_backward(gpu, pg1):
    """bf16 parameters with the default split master through a real backward: the fresh gradients
    are read where backward left them, by the norm pass and by the update.  W1 spans two chunks of
    4,096 and a partial one."""
    from oracle import c_oracle
    from zero_amd import zero2

    torch.manual_seed(0)
    w1 = torch.nn.Parameter((torch.randn(96, 96) * 0.1).to(torch.bfloat16).to(gpu))
    b1 = torch.nn.Parameter((torch.randn(96) * 0.1).to(torch.bfloat16).to(gpu))
    w2 = torch.nn.Parameter((torch.randn(96, 7) * 0.1).to(torch.bfloat16).to(gpu))
    params = [w1, b1, w2]
    assert w1.numel() == 2 * 4096 + 1024
    x = torch.randn(32, 96).to(torch.bfloat16).to(gpu)
    y = torch.randn(32, 7).to(torch.bfloat16).to(gpu)
    host = lambda t: t.detach().cpu().contiguous().view(torch.int16).numpy().reshape(-1).view(np.uint16).copy()  # noqa: E731
    ref = []
    for p in params:
        master0 = zo.bf16_bits_to_f32(host(p))
        ref.append(_ref_init("split", p.numel(), master0, False))
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), max_grad_norm=1.0)
    assert opt.engine.split and opt.engine.inplace
    coefs = []
    for t, scale in enumerate(SCALES, 1):
        opt.zero_grad()
        loss = (((torch.tanh(x @ w1 + b1) @ w2) - y) ** 2).sum() * scale
        loss.backward()
        gbits = [host(p.grad) for p in params]
        norm = _norm64([zo.bf16_bits_to_f32(g) for g in gbits])
        if t == 1:
            opt.max_grad_norm = 4.0 * norm  # (a plain attribute: changed between steps)
        opt.step()
        assert opt.engine.inplace_reads == len(params)
        assert abs(float(opt.last_grad_norm.item()) - norm) <= 1e-6 * norm
        coef = _f32(opt.last_clip_coef)
        coefs.append(coef)
        hp = c_oracle.hparams(step=t, grad_div=1.0)
        for p, r, g in zip(params, ref, gbits):
            _ref_step("split", r, [(0, p.numel(), True)], g, 1.0, coef, hp)
            st = opt.optimizer.state[p]
            got = {"hi": host(p), "lo": host(st["master_residual"]),
                   "m": st["exp_avg"].cpu().numpy().reshape(-1), "v": st["exp_avg_sq"].cpu().numpy().reshape(-1)}
            for name in got:
                bad = np.flatnonzero(_bits(got[name]) != _bits(r[name]))
                assert bad.size == 0, f"step {t} {name}: {bad.size} differ, first at {bad[:8]}"
    print("coefficients", coefs)
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE
    assert 0.05 < coefs[1] < 0.2


def test_inf_equals_none(gpu, pg1):
    """max_grad_norm=inf reports the norm and changes nothing: parameters and state bit-identical
    to the unclipped path, which allocates no clipping buffers."""
    from zero_amd import zero1

    shapes = [(130, 33), (5,), (2049,)]
    rng = np.random.default_rng(4)
    init = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    steps = [_grads(rng, shapes, s) for s in SCALES]
    out = {}
    for limit in (None, float("inf")):
        params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(gpu)) for a in init]
        opt = zero1.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3, amsgrad=True),
                                     max_grad_norm=limit)
        for grads in steps:
            opt.zero_grad()
            for p, g in zip(params, grads):
                p.grad = torch.from_numpy(g).to(gpu)
            opt.step()
            if limit is None:
                assert opt.last_grad_norm is None and opt.engine.clip_out is None
                assert opt.last_norm_bytes == 0 and not hasattr(opt.engine, "clip_partials")
            else:
                want = _norm64(grads)
                assert abs(float(opt.last_grad_norm.item()) - want) <= 1e-6 * want
                assert _f32(opt.last_clip_coef).view(np.uint32) == ONE
        out[limit] = [a for p in params for a in (
            p.detach().cpu().numpy(), *(opt.optimizer.state[p][k].cpu().numpy()
                                        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")))]
    for a, b in zip(out[None], out[float("inf")]):
        assert np.array_equal(_bits(a.reshape(-1)), _bits(b.reshape(-1)))


def test_construction_errors(gpu, pg1):
    from zero_amd import zero2

    mk = lambda: torch.optim.Adam([torch.nn.Parameter(torch.zeros(8, device=gpu))], lr=1e-3)  # noqa: E731
    with pytest.raises(ValueError, match="overlap"):
        zero2.ShardedOptimizer(mk(), max_grad_norm=1.0, overlap=True)
    with pytest.raises(ValueError, match="bucket"):
        zero2.ShardedOptimizer(mk(), max_grad_norm=1.0, arena="buckets")
    for bad in (-1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="max_grad_norm"):
            zero2.ShardedOptimizer(mk(), max_grad_norm=bad)
    opt = zero2.ShardedOptimizer(mk(), arena="buckets")  # unclipped: as before
    opt.max_grad_norm = 1.0
    opt.params[0].grad = torch.ones(8, device=gpu)
    with pytest.raises(ValueError, match="bucket"):
        opt.step()


# ---------------------------------------------------------------------------------------------
# world size 2 through real RCCL
# ---------------------------------------------------------------------------------------------
def _same_norm_on_every_rank(opt, ws):
    every = [None] * ws
    dist.all_gather_object(every, int(_f32(opt.last_grad_norm).view(np.uint32)))
    assert len(set(every)) == 1, every


def _ws2_fp32_worker(rank, ws, port, shapes, groups):
    """ZeRO-2 fp32 against the CPU replica on (g0 + g1) / 2; 64-element windows, so several rounds.
    With one parameter rank 1 owns nothing: it contributes 0 to the scalar all-reduce, takes part
    in it and reaches the end."""
    from _gloo_comm import test_comm
    from zero_amd import zero2

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(12)
    init = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    local = [[_grads(rng, shapes, s) for _ in range(ws)] for s in SCALES]  # [step][rank][param]
    avg = [[((a + b) / np.float32(2)).astype(np.float32) for a, b in zip(*per_rank)] for per_rank in local]
    max_norm = 4.0 * _norm64(avg[0])
    rep = _Replica(init, groups)
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in init]
    opt = zero2.ShardedOptimizer(
        torch.optim.AdamW([dict(params=[params[i] for i in idx], **kw) for idx, kw in groups]),
        comm=test_comm(), bucket_mb=ws * 64 * 4 / (1 << 20), max_grad_norm=max_norm)
    if len(shapes) == 1:
        assert (rank == 1) == (len(opt.local_param_indices) == 0)
    coefs = []
    for t in range(len(SCALES)):
        opt.zero_grad()
        for p, g in zip(params, local[t][rank]):
            set_grad(p, torch.from_numpy(g).to(dev))
        opt.step()
        want = rep.step(avg[t], max_norm)
        assert abs(float(opt.last_grad_norm.item()) - want) <= 1e-6 * want
        coefs.append(_f32(opt.last_clip_coef))
        _same_norm_on_every_rank(opt, ws)
        _compare_fp32(opt, params, rep, owned=opt.local_param_indices)
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE and 0.05 < coefs[1] < 0.2
    dist.destroy_process_group()


def _ws2_split_worker(rank, ws, port):
    """ZeRO-2 bf16 with the split master, bit for bit against the oracle: the reduced gradient is
    the bf16 rounding (nearest even) of the two-term fp32 sum, the coefficient the device's."""
    from _gloo_comm import test_comm
    from oracle import c_oracle
    from zero_amd import zero2

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    shapes = [(100, 90), (64,), (4096 + 40,)]
    rng = np.random.default_rng(13)
    init = [zo.f32_to_bf16_bits((rng.standard_normal(s) * 0.05).astype(np.float32)).reshape(-1) for s in shapes]
    dev_bf16 = lambda bits, s: torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16).reshape(s).to(dev)  # noqa: E731
    host = lambda t: t.detach().cpu().contiguous().view(torch.int16).numpy().reshape(-1).view(np.uint16).copy()  # noqa: E731
    params = [torch.nn.Parameter(dev_bf16(a, s)) for a, s in zip(init, shapes)]
    ref = [_ref_init("split", a.size, zo.bf16_bits_to_f32(a), False) for a in init]
    local = [[[zo.f32_to_bf16_bits(g).reshape(-1) for g in _grads(rng, shapes, s)] for _ in range(ws)]
             for s in SCALES]
    reduced = [[zo.f32_to_bf16_bits(zo.bf16_bits_to_f32(a) + zo.bf16_bits_to_f32(b))
                for a, b in zip(*per_rank)] for per_rank in local]
    max_norm = 4.0 * _norm64([zo.bf16_bits_to_f32(g) for g in reduced[0]]) / 2.0
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), comm=test_comm(),
                                 bucket_mb=ws * 4096 * 2 / (1 << 20), max_grad_norm=max_norm)
    assert opt.engine.split and opt.engine.K > 1
    coefs = []
    for t in range(len(SCALES)):
        opt.zero_grad()
        for p, g, s in zip(params, local[t][rank], shapes):
            set_grad(p, dev_bf16(g, s))
        opt.step()
        want = _norm64([zo.bf16_bits_to_f32(g) for g in reduced[t]]) / 2.0
        assert abs(float(opt.last_grad_norm.item()) - want) <= 1e-6 * want
        coef = _f32(opt.last_clip_coef)
        coefs.append(coef)
        _same_norm_on_every_rank(opt, ws)
        hp = c_oracle.hparams(step=t + 1, grad_div=1.0)
        for i, (p, r) in enumerate(zip(params, ref)):
            _ref_step("split", r, [(0, p.numel(), True)], reduced[t][i], 2.0, coef, hp)
            got = {"hi": host(p)}
            if i in opt.local_param_indices:
                st = opt.optimizer.state[p]
                got.update(lo=host(st["master_residual"]), m=st["exp_avg"].cpu().numpy().reshape(-1),
                           v=st["exp_avg_sq"].cpu().numpy().reshape(-1))
            for name in got:
                bad = np.flatnonzero(_bits(got[name]) != _bits(r[name]))
                assert bad.size == 0, f"rank {rank} step {t} param {i} {name}: {bad.size} differ"
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE and 0.05 < coefs[1] < 0.2
    dist.destroy_process_group()


def _ws2_zero1_refused_worker(rank, ws, port):
    """ZeRO-1 at world size 2 with max_grad_norm: ValueError on every rank, before any collective
    (no communicator is passed; had the constructor gone on, it would have built one)."""
    from zero_amd import zero1

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    p = torch.nn.Parameter(torch.zeros(8, device="cuda:0"))
    with pytest.raises(ValueError, match="ZeRO-1"):
        zero1.ShardedOptimizer(torch.optim.Adam([p], lr=1e-3), max_grad_norm=1.0)
    dist.destroy_process_group()


def test_ws2_rccl(gpu, rccl_env):
    two_groups = [([0], dict(lr=1e-3, weight_decay=1e-2)), ([1, 2], dict(lr=2e-3, weight_decay=0.0))]
    t0 = time.perf_counter()
    spawn_batch(2, [(_ws2_fp32_worker, ([(70, 33), (0,), (130,)], two_groups)),
                    (_ws2_split_worker, ()),
                    (_ws2_fp32_worker, ([(37, 9)], [([0], dict(lr=1e-3, weight_decay=0.0))])),
                    (_ws2_zero1_refused_worker, ())], all_spawned=True)
    print(f"ws=2 clipping batch: {time.perf_counter() - t0:.1f} s")
