"""``skip_nonfinite=True``: a step whose gradient norm is not finite is skipped on the device.

ZeRO-3 at world size 2 through real RCCL and ZeRO-2 on the flat arena at world size 1, both with
the bf16 split master.  Step 1 is finite; in step 2 one element of one rank's local gradient is
+inf or NaN (ZeRO-3: rank 1's, in a row whose reduced chunk lands on rank 0, so rank 1 learns of
it through the scalar all-reduce alone); step 3 is finite.  After step 2 every parameter and every
state view is byte-identical to after step 1 on every rank, the counter is 1, the coefficient NaN
and the norm not finite.  After step 3 they equal the oracle applied to the state of step 1 with
the hyper-parameters of step count 3: the host's counts advance through a skipped step, the
deviation DESIGN.md §6 records.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _clip_inputs as ci
from _zero_run import spawn_batch
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_clip_optimizer import pg1, rccl_env  # noqa: F401
from test_gpu_gradnorm import _bits, _ref_init, _ref_step
from test_gpu_zero3_accumulate import _rows
from test_gpu_zero3_clip import ONE, _Ref, _build, _f32, _norm64, host

pytestmark = pytest.mark.gpu

BAD = {"inf": np.inf, "nan": np.nan}


def _snapshot(params, views_of):
    return [(host(p), {k: host(v) for k, v in views_of(i).items()}) for i, p in enumerate(params)]


def _unchanged(params, views_of, before, what):
    for i, p in enumerate(params):
        assert np.array_equal(host(p), before[i][0]), f"{what}: param {i} moved"
        for k, v in views_of(i).items():
            assert np.array_equal(host(v), before[i][1][k]), f"{what}: {k} of param {i} moved"


def _skipped(opt, n, what):
    assert int(opt.skipped_steps.item()) == n and opt.skipped_steps.dim() == 0, what
    assert opt.skipped_steps.dtype == torch.int64


def _skip_zero3(rank, ws, dev, comm, bad):
    shapes, ranks = ci.SHAPES, list(range(ws))
    model, params, opt, init = _build(dev, "bf16", comm, shapes, max_grad_norm=1.0,
                                      skip_nonfinite=True)
    ar = opt._arena
    ref = [_Ref(_rows(w, shapes[i], ws, rank), "bf16", "f32", False, int(ar.slot[i]))
           for i, w in enumerate(init)]
    assert opt.skipped_steps is None  # (before the first step)
    before = None
    for step in range(3):
        for k, m in enumerate(model.probes):
            c = ci.local(step, 0, rank, k, "bf16").copy()
            if step == 1 and rank == 1 and k == 0:
                c[0, 5] = BAD[bad]  # row 0: rank 0's chunk
            m.c = torch.from_numpy(c).to(dev, torch.bfloat16)
        model([True] * len(shapes)).backward()
        grads = [ci.reduced(step, 0, i, ranks, "bf16") for i in range(len(shapes))]
        if step == 0:
            opt.max_grad_norm = 4.0 * _norm64(grads, ws, rank, False, shapes)
        opt.step()
        torch.cuda.synchronize()
        what = f"rank {rank} step {step} ({bad})"
        assert [int(s) for s in opt._steps] == [(step + 1) * int(n > 0) for n in ar.ln], what
        if step == 1:
            _unchanged(params, opt._state_views, before, what)
            _skipped(opt, 1, what)
            assert np.isnan(_f32(opt.last_clip_coef)) and not np.isfinite(_f32(opt.last_grad_norm))
            for r in ref:
                r.t += 1  # the host's count advances; nothing else does
            continue
        coef = _f32(opt.last_clip_coef)
        assert coef.view(np.uint32) == ONE, what
        _skipped(opt, int(step > 1), what)
        for i, (p, r) in enumerate(zip(params, ref)):
            if int(ar.ln[i]):
                r.step(_rows(grads[i], shapes[i], ws, rank), float(ws), coef)
                assert r.t == step + 1
                r.check(p, opt.optimizer.state[p], f"{what} param {i}")
        before = _snapshot(params, opt._state_views)
    every = [None] * ws
    dist.all_gather_object(every, int(opt.skipped_steps.item()))
    assert every == [1] * ws


def test_zero3_ws2_rccl(gpu, rccl_env):
    spawn_batch(2, [(_mr, ("_skip_zero3", "inf")), (_mr, ("_skip_zero3", "nan"))], all_spawned=True)


def _mr(rank, ws, port, fn, *args):
    import faulthandler
    import sys

    from _gloo_comm import test_comm
    from _zero_run import init_pg

    if rank:
        faulthandler.dump_traceback_later(120, exit=True, file=sys.stderr)
    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    globals()[fn](rank, ws, torch.device("cuda:0"), test_comm(), *args)
    dist.barrier()
    dist.destroy_process_group()
    if rank:
        faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("bad", list(BAD))
def test_zero2_flat_ws1(gpu, pg1, bad):
    """ZeRO-2 on the flat arena with max_grad_norm=inf: a pure skip, nothing is clipped."""
    from zero_amd import zero2

    shapes = [(96, 96), (96,), (96, 7)]
    rng = np.random.default_rng(21)
    bits16 = lambda s, scale: zo.f32_to_bf16_bits((rng.standard_normal(s) * scale).astype(np.float32)).reshape(-1)  # noqa: E731
    dev_bf16 = lambda b, s: torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16).reshape(s).to(gpu)  # noqa: E731
    init = [bits16(s, 0.05) for s in shapes]
    grads = [[bits16(s, 1e-2) for s in shapes] for _ in range(3)]
    grads[1][0][7] = zo.f32_to_bf16_bits(np.array([BAD[bad]], np.float32))[0]
    params = [torch.nn.Parameter(dev_bf16(a, s)) for a, s in zip(init, shapes)]
    ref = [_ref_init("split", a.size, zo.bf16_bits_to_f32(a), False) for a in init]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), max_grad_norm=float("inf"),
                                 skip_nonfinite=True)
    assert opt.engine.split and opt.skipped_steps is None
    views_of = lambda i: {k: v for k, v in opt.optimizer.state[params[i]].items()  # noqa: E731
                          if k != "step"}
    before = None
    for t in range(3):
        opt.zero_grad()
        for p, g, s in zip(params, grads[t], shapes):
            p.grad = dev_bf16(g, s)
        opt.step()
        torch.cuda.synchronize()
        assert [int(s) for s in opt.engine.steps] == [t + 1] * len(params)
        if t == 1:
            _unchanged(params, views_of, before, f"step {t} ({bad})")
            _skipped(opt, 1, bad)
            assert np.isnan(_f32(opt.last_clip_coef)) and not np.isfinite(_f32(opt.last_grad_norm))
            continue
        assert _f32(opt.last_clip_coef).view(np.uint32) == ONE
        _skipped(opt, int(t > 1), bad)
        hp = c_oracle.hparams(step=t + 1, grad_div=1.0)
        for i, (p, r, g) in enumerate(zip(params, ref, grads[t])):
            _ref_step("split", r, [(0, p.numel(), True)], g, 1.0, np.float32(1.0), hp)
            st = opt.optimizer.state[p]
            got = {"hi": host(p), "lo": host(st["master_residual"]),
                   "m": host(st["exp_avg"]), "v": host(st["exp_avg_sq"])}
            for name in got:
                bad_at = np.flatnonzero(got[name] != _bits(r[name]))
                assert bad_at.size == 0, f"step {t} param {i} {name}: {bad_at.size} differ"
        before = _snapshot(params, views_of)


def test_constructor_refusals(gpu, pg1):
    from zero_amd import zero2, zero3

    P = lambda: [torch.nn.Parameter(torch.zeros(8, device=gpu))]  # noqa: E731
    for mk in (lambda **kw: zero2.ShardedOptimizer(torch.optim.Adam(P()), **kw),
               lambda **kw: zero3.ShardedOptimizer(torch.optim.Adam(P()), update=True, **kw)):
        with pytest.raises(ValueError, match="max_grad_norm"):
            mk(skip_nonfinite=True)
        opt = mk(skip_nonfinite=True, max_grad_norm=float("inf"))
        opt.max_grad_norm = None  # (re-checked at every step)
        opt.params[0].grad = torch.ones(8, device=gpu)
        with pytest.raises(ValueError, match="max_grad_norm"):
            opt.step()
    for mk in (lambda **kw: zero2.ShardedOptimizer(torch.optim.SGD(P(), lr=0.1, momentum=0.9), **kw),
               lambda **kw: zero3.ShardedOptimizer(torch.optim.SGD(P(), lr=0.1, momentum=0.9),
                                                   update=True, **kw)):
        with pytest.raises(ValueError, match="SGD"):
            mk(skip_nonfinite=True, max_grad_norm=1.0)
        mk(max_grad_norm=1.0)  # clipping alone: supported
