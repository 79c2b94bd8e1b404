"""``ShardedOptimizer(..., max_grad_norm=m, param_grad_norms=True)``: ``last_param_grad_norms``, the
L2 norm of every parameter's averaged gradient, out of the clipping pass — ZeRO-1/2 on the flat
arena and ZeRO-3 update mode, at world size 1 and at world size 2 (gloo-staged).

Every entry is held to float64 of the gradient the update reads (torch's ``g.double().norm()`` on
the CPU: its own error is below 1e-15).  The bound is DESIGN.md §4's: (K + 2) * 2^-24 relative on
a parameter's sum of squares (K = 16 fp32 terms per lane and chunk for the split master, 8
otherwise), plus (ws - 1) * 2^-24 where the all-reduce adds the ranks' chunk sums (ZeRO-3); the
norm has half of that plus 2^-24 for its own rounding.  Trajectories, global norm and coefficients
are checked as tests/test_gpu_clip_optimizer.py checks them, with its replica.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _clip_inputs as ci
import test_gpu_zero3_clip as z3c
from _zero_run import init_pg, set_grad, spawn_batch
from test_abi_param_norms import param_norms_ref
from test_gpu_clip_optimizer import (ONE, SCALES, _compare_fp32, _f32, _grads, _norm64, _Replica,
                                     pg1)  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _bound(k_terms, ws_sum=1):
    """Relative bound on a reported norm: half the sum of squares' bound, plus its own rounding."""
    return ((k_terms + 2) + (ws_sum - 1)) * U / 2 + U


def _norms64(grads, div=1.0):
    """float64 L2 norm per gradient (None or 0-size: 0) over ``div``."""
    return [0.0 if g is None or np.size(g) == 0
            else float(torch.from_numpy(np.ascontiguousarray(g, np.float64)).norm()) / div
            for g in grads]


def _check_vec(vec, want, bound, what):
    got = vec.cpu().numpy()
    assert vec.dim() == 1 and vec.dtype == torch.float32 and len(got) == len(want)
    worst = 0.0
    for i, (a, w) in enumerate(zip(got, want)):
        if w == 0.0:
            assert a.view(np.uint32) == 0, f"{what} entry {i}: {a!r}, not +0.0"
            continue
        assert np.isfinite(a), (what, i)
        worst = max(worst, abs(float(a) - w) / w)
    print(f"{what}: worst rel {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound, what
    return got


def _sumsq_is_consistent(clip, opt, ws):
    """The vector's last element is the sum of squares ``last_grad_norm`` was computed from."""
    ss = clip.reduced.cpu().numpy()
    assert len(ss) == len(opt.params) + 1 and clip.sumsq.data_ptr() == clip.reduced[-1:].data_ptr()
    want = param_norms_ref(ss[-1:], float(ws))[0]
    assert want.view(np.uint32) == _f32(opt.last_grad_norm).view(np.uint32)
    norms = opt.last_param_grad_norms.cpu().numpy()
    assert np.array_equal(norms.view(np.uint32), param_norms_ref(ss[:-1], float(ws)).view(np.uint32))


def _same_on_every_rank(opt, ws):
    every = [None] * ws
    dist.all_gather_object(every, opt.last_param_grad_norms.cpu().numpy().view(np.uint32).tolist())
    assert all(e == every[0] for e in every), every


# ---------------------------------------------------------------------------------------------
# world size 1
# ---------------------------------------------------------------------------------------------
def test_ws1_fp32_two_groups(gpu, pg1):
    """tests/test_gpu_clip_optimizer.py's case with the option: two AdamW groups, a 0-size
    parameter, one parameter without a gradient in step 2; norm, coefficients and trajectory as
    there, and every entry of the vector."""
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
        max_grad_norm=max_norm, param_grad_norms=True)
    assert opt.last_param_grad_norms is None
    coefs, seen = [], None
    for t, grads in enumerate(steps):
        opt.zero_grad()
        for p, g in zip(params, grads):
            if g is not None:
                p.grad = torch.from_numpy(g).to(gpu)
        opt.step()
        want_vec = _norms64(grads)  # (before the replica: clip_grad_norm_ scales them in place)
        want = rep.step(grads, max_norm)
        got = float(opt.last_grad_norm.item())
        assert abs(got - want) <= 1e-6 * want
        coefs.append(_f32(opt.last_clip_coef))
        assert opt.last_norm_bytes == 4 * sum(g.size for g in grads if g is not None)
        _compare_fp32(opt, params, rep, owned=range(len(params)))
        vec = opt.last_param_grad_norms
        assert seen is None or vec is seen  # the same tensor every step
        seen = vec
        got = _check_vec(vec, want_vec, _bound(8), f"step {t}")
        assert got[2].view(np.uint32) == 0 and (t != 1 or got[3].view(np.uint32) == 0)
        _sumsq_is_consistent(opt.engine.clip, opt, 1)
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE
    assert 0.05 < coefs[1] < 0.2


def test_ws1_bf16_split_through_backward(gpu, pg1):
    """bf16 parameters, split master, a real backward: the entries against float64 of the bf16
    gradients backward left (W1 spans two chunks of 4,096 and a partial one)."""
    from zero_amd import zero2

    torch.manual_seed(0)
    w1 = torch.nn.Parameter((torch.randn(96, 96) * 0.1).to(torch.bfloat16).to(gpu))
    b1 = torch.nn.Parameter((torch.randn(96) * 0.1).to(torch.bfloat16).to(gpu))
    w2 = torch.nn.Parameter((torch.randn(96, 7) * 0.1).to(torch.bfloat16).to(gpu))
    params = [w1, b1, w2]
    x = torch.randn(32, 96).to(torch.bfloat16).to(gpu)
    y = torch.randn(32, 7).to(torch.bfloat16).to(gpu)
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), max_grad_norm=1.0,
                                 param_grad_norms=True)
    assert opt.engine.split and opt.engine.inplace
    for t, scale in enumerate(SCALES):
        opt.zero_grad()
        loss = (((torch.tanh(x @ w1 + b1) @ w2) - y) ** 2).sum() * scale
        loss.backward()
        grads = [p.grad.detach().double().cpu().numpy() for p in params]
        norm = _norm64(grads)
        opt.step()
        assert abs(float(opt.last_grad_norm.item()) - norm) <= 1e-6 * norm
        _check_vec(opt.last_param_grad_norms, _norms64(grads), _bound(16), f"step {t}")
        _sumsq_is_consistent(opt.engine.clip, opt, 1)


def test_skip_nonfinite_names_the_parameter(gpu, pg1):
    """A NaN planted in one parameter's gradient: the step is skipped (``skipped_steps`` 1, no
    parameter or moment changes) and the vector shows which parameter carried it."""
    from zero_amd import zero2

    shapes = [(50, 40), (33,), (2049,)]
    rng = np.random.default_rng(7)
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(gpu))
              for s in shapes]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), max_grad_norm=1.0,
                                 skip_nonfinite=True, param_grad_norms=True)

    def step(grads):
        opt.zero_grad()
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g).to(gpu)
        opt.step()
        torch.cuda.synchronize()

    def snapshot():
        return [a.detach().cpu().numpy().copy() for p in params
                for a in (p, opt.optimizer.state[p]["exp_avg"], opt.optimizer.state[p]["exp_avg_sq"])]

    grads = _grads(rng, shapes, 1.0)
    step(grads)
    assert int(opt.skipped_steps.item()) == 0
    _check_vec(opt.last_param_grad_norms, _norms64(grads), _bound(8), "finite step")
    before = snapshot()
    bad = _grads(rng, shapes, 1.0)
    bad[1][17] = np.nan
    step(bad)
    assert int(opt.skipped_steps.item()) == 1 and np.isnan(_f32(opt.last_clip_coef))
    got = opt.last_param_grad_norms.cpu().numpy()
    assert np.isnan(got[1]) and np.isfinite(got[0]) and np.isfinite(got[2])
    want = _norms64(bad)
    for i in (0, 2):
        assert abs(float(got[i]) - want[i]) <= _bound(8) * want[i]
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _one_step(gpu, mk_params, mk_opt, grads, **kw):
    params = mk_params()
    opt = mk_opt(params, **kw)
    opt.zero_grad()
    for p, g in zip(params, grads):
        p.grad = g.clone()
    opt.step()
    torch.cuda.synchronize()
    return params, opt


def _raw(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().copy()


def test_sgd_momentum_and_master_none(gpu, pg1):
    """One step each of SGD with momentum (fp32) and of Adam with master="none" (bf16): the vector
    is right, and with max_grad_norm=inf the update has the bits of the run without the option."""
    from zero_amd import zero2

    shapes = [(70, 33), (5,), (4096 + 36,)]
    rng = np.random.default_rng(9)
    init = [rng.standard_normal(s).astype(np.float32) * 0.1 for s in shapes]
    g32 = _grads(rng, shapes, 1.0)
    cases = {
        "sgd": (torch.float32, 8, "momentum_buffer",
                lambda ps, **kw: zero2.ShardedOptimizer(torch.optim.SGD(ps, lr=0.05, momentum=0.9), **kw)),
        "master-none": (torch.bfloat16, 16, "exp_avg",
                        lambda ps, **kw: zero2.ShardedOptimizer(torch.optim.Adam(ps, lr=1e-3),
                                                                master="none", state_seed=11, **kw)),
    }
    for name, (dt, k_terms, state, mk_opt) in cases.items():
        mk_params = lambda: [torch.nn.Parameter(torch.from_numpy(a.copy()).to(gpu, dt)) for a in init]  # noqa: E731
        grads = [torch.from_numpy(g).to(gpu, dt) for g in g32]
        runs = [_one_step(gpu, mk_params, mk_opt, grads, max_grad_norm=float("inf"), **kw)
                for kw in ({}, dict(param_grad_norms=True))]
        (p0, o0), (p1, o1) = runs
        assert o0.last_param_grad_norms is None
        assert _f32(o1.last_clip_coef).view(np.uint32) == ONE
        assert _f32(o0.last_grad_norm) == pytest.approx(float(_f32(o1.last_grad_norm)), rel=2 * _bound(k_terms))
        _check_vec(o1.last_param_grad_norms, _norms64([g.double().cpu().numpy() for g in grads]),
                   _bound(k_terms), name)
        for a, b in zip(p0, p1):
            assert np.array_equal(_raw(a), _raw(b)), name
            assert np.array_equal(_raw(o0.optimizer.state[a][state]), _raw(o1.optimizer.state[b][state])), name


def test_refusals(gpu, pg1):
    """Without max_grad_norm the option is a ValueError, at construction and when the limit is
    taken away between steps; what refuses max_grad_norm refuses it with the option as before."""
    from zero_amd import zero1, zero2, zero3

    P = lambda: [torch.nn.Parameter(torch.zeros(8, device=gpu))]  # noqa: E731
    for mod, kw in ((zero1, {}), (zero2, {}), (zero3, dict(update=True))):
        with pytest.raises(ValueError, match="param_grad_norms=True .* needs max_grad_norm"):
            mod.ShardedOptimizer(torch.optim.Adam(P(), lr=1e-3), param_grad_norms=True, **kw)
        params = P()
        opt = mod.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), max_grad_norm=1.0,
                                   param_grad_norms=True, **kw)
        opt.max_grad_norm = None
        params[0].grad = torch.ones(8, device=gpu)
        with pytest.raises(ValueError, match="param_grad_norms"):
            opt.step()
    with pytest.raises(ValueError, match="max_grad_norm is not supported with overlap"):
        zero2.ShardedOptimizer(torch.optim.Adam(P()), max_grad_norm=1.0, overlap=True, param_grad_norms=True)
    with pytest.raises(ValueError, match="max_grad_norm is not supported with arena='buckets'"):
        zero2.ShardedOptimizer(torch.optim.Adam(P()), max_grad_norm=1.0, arena="buckets",
                               param_grad_norms=True)
    with pytest.raises(ValueError, match="max_grad_norm applies to update mode"):
        zero3.ShardedOptimizer(torch.optim.Adam(P()), update=False, max_grad_norm=1.0,
                               param_grad_norms=True)
    with pytest.raises(ValueError, match="skip_nonfinite=True is not supported with torch.optim.SGD"):
        zero2.ShardedOptimizer(torch.optim.SGD(P(), lr=0.1), max_grad_norm=1.0, skip_nonfinite=True,
                               param_grad_norms=True)
    for bad in (-1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="max_grad_norm must be"):
            zero2.ShardedOptimizer(torch.optim.Adam(P()), max_grad_norm=bad, param_grad_norms=True)


# ---------------------------------------------------------------------------------------------
# world size 2, gloo-staged
# ---------------------------------------------------------------------------------------------
def _ws2_zero2_worker(rank, ws, port):
    """ZeRO-2 fp32 on the flat arena with 64-element windows: (70, 33) is cut across 37 rounds;
    parameter 3 is frozen (it belongs to rank 1).  Entries = the norm of (g0 + g1) / 2."""
    from _gloo_comm import test_comm
    from zero_amd import zero2

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    shapes = [(70, 33), (0,), (130,), (9, 5), (77,)]
    groups = [([0, 1], dict(lr=1e-3, weight_decay=1e-2)), ([2, 3, 4], dict(lr=2e-3, weight_decay=0.0))]
    frozen = 3
    rng = np.random.default_rng(12)
    init = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    local = [[_grads(rng, shapes, s) for _ in range(ws)] for s in SCALES]  # [step][rank][param]
    summed = [[None if i == frozen else (a + b).astype(np.float32)
               for i, (a, b) in enumerate(zip(*per_rank))] for per_rank in local]
    avg = [[None if g is None else (g / np.float32(2)).astype(np.float32) for g in s] for s in summed]
    max_norm = 4.0 * _norm64(avg[0])
    rep = _Replica(init, groups)
    rep.params[frozen].requires_grad_(False)
    params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev), requires_grad=i != frozen)
              for i, a in enumerate(init)]
    opt = zero2.ShardedOptimizer(
        torch.optim.AdamW([dict(params=[params[i] for i in idx], **kw) for idx, kw in groups]),
        comm=test_comm(), bucket_mb=ws * 64 * 4 / (1 << 20), max_grad_norm=max_norm,
        param_grad_norms=True)
    assert opt.engine.K > 1 and (frozen in opt.local_param_indices) == (rank == 1)
    coefs = []
    for t in range(len(SCALES)):
        opt.zero_grad()
        for i, (p, g) in enumerate(zip(params, local[t][rank])):
            if i != frozen:
                set_grad(p, torch.from_numpy(g).to(dev))
        opt.step()
        want = rep.step(avg[t], max_norm)
        assert abs(float(opt.last_grad_norm.item()) - want) <= 1e-6 * want
        coefs.append(_f32(opt.last_clip_coef))
        # the pass reads the sums; the division by the world size follows the square root
        got = _check_vec(opt.last_param_grad_norms, _norms64(summed[t], 2.0), _bound(8),
                         f"rank {rank} step {t}")
        assert got[frozen].view(np.uint32) == 0
        _same_on_every_rank(opt, ws)
        _sumsq_is_consistent(opt.engine.clip, opt, ws)
        _compare_fp32(opt, [p for i, p in enumerate(params)], rep,
                      owned=[i for i in opt.local_param_indices if i != frozen])
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE and 0.05 < coefs[1] < 0.2
    dist.destroy_process_group()


def _ws2_zero1_refused_worker(rank, ws, port):
    from zero_amd import zero1

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    p = torch.nn.Parameter(torch.zeros(8, device="cuda:0"))
    with pytest.raises(ValueError, match="max_grad_norm is not supported with ZeRO-1"):
        zero1.ShardedOptimizer(torch.optim.Adam([p], lr=1e-3), max_grad_norm=1.0, param_grad_norms=True)
    dist.destroy_process_group()


def _ws2_zero3_worker(rank, ws, port, passes):
    """ZeRO-3 update mode on tests/_clip_inputs.py's shapes — (7, 24) in chunks of 4 and 3 rows,
    (1,) with an empty chunk on rank 1 — the entries being the norm over both ranks' chunks.
    ``passes`` 2: bf16 parameters with grad_accumulation and accumulation_dtype=float32, the pass
    reading the fp32 accumulation arena."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    shapes = ci.SHAPES
    pdt = "bf16" if passes > 1 else "f32"
    arena, widen = ("bf16", True) if passes > 1 else ("f32", False)
    kw = dict(max_grad_norm=1.0, param_grad_norms=True)
    if passes > 1:
        kw.update(grad_accumulation=True, accumulation_dtype=torch.float32)
    model, params, opt, _ = z3c._build(dev, pdt, test_comm(), shapes, None, **kw)
    assert int(opt._arena.ln[3]) == (1 if rank == 0 else 0)
    assert opt.last_param_grad_norms is None
    coefs = []
    for step in range(len(ci.SCALES)):
        for pas in range(passes):
            z3c._backward(model, step, pas, rank, arena, dev, shapes)
        grads = [ci.values(ci.accumulated(step, passes, i, list(range(ws)), arena, widen, shapes))
                 for i in range(len(shapes))]
        want = _norms64(grads, float(ws))
        total = _norm64(grads) / ws
        if step == 0:
            opt.max_grad_norm = 4.0 * total
        opt.step()
        torch.cuda.synchronize()
        assert abs(float(opt.last_grad_norm.item()) - total) <= 1e-6 * total
        coefs.append(_f32(opt.last_clip_coef))
        _check_vec(opt.last_param_grad_norms, want, _bound(16 if passes > 1 else 8, ws),
                   f"rank {rank} passes {passes} step {step}")
        _same_on_every_rank(opt, ws)
        _sumsq_is_consistent(opt._clip, opt, ws)
    assert coefs[0].view(np.uint32) == ONE and coefs[2].view(np.uint32) == ONE and 0.05 < coefs[1] < 0.2
    dist.barrier()
    dist.destroy_process_group()


def test_ws2_gloo(gpu):
    spawn_batch(2, [(_ws2_zero2_worker, ()), (_ws2_zero3_worker, (1,)), (_ws2_zero3_worker, (2,)),
                    (_ws2_zero1_refused_worker, ())])
