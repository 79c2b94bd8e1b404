"""``ShardedOptimizer(..., param_update_norms=True)``: ``last_param_update_norms`` and
``last_param_weight_norms``, the L2 norms of every parameter's update and weights on the fp32
master, out of the fused Adam update -- ZeRO-1/2 on the flat arena and ZeRO-3 update mode, at world
size 1 and at world size 2 (gloo-staged).

Every entry is held to float64 of master snapshots taken around the step through
``optimizer.state`` (``join_split_master`` for the split master; the parameter itself where it is
fp32): d = after - before as one float32 subtraction, the sums of d^2 and of after^2 in float64, at
world size 2 added over the ranks' shares.  The bound is DESIGN.md §4's: (K + 2) * 2^-24 relative
on a parameter's sum (K = 16 fp32 terms per lane and chunk for the split master, 8 otherwise), plus
(ws - 1) * 2^-24 where the all-reduce adds the ranks' chunk sums (ZeRO-3); a norm has half of that
plus 2^-24 for its own rounding.

The models are probes (tests/_clip_inputs.py): forward = (weight * c).sum(), so backward leaves
exactly c as the gradient; the steps are scaled x1, x40 and x0.05, which with ``max_grad_norm`` at
four times the first norm clips the second step alone.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _clip_inputs as ci
import test_gpu_zero3_clip as z3c
from _zero_run import init_pg, module_for, spawn_batch
from test_gpu_clip_optimizer import pg1  # noqa: F401
from test_gpu_zero3_accumulate import Probe, ProbeModel

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF16 = torch.bfloat16
# (66, 128): two chunks of 4,096 and a partial one; (4096 + 37,): a chunk, a group and a tail
SHAPES = [(66, 128), (7, 24), (16,), (1,), (4096 + 37,)]
GROUPS = [([0, 1, 2], dict(lr=1e-3, weight_decay=1e-2)), ([3, 4], dict(lr=2e-3, weight_decay=0.0))]
STEPS = len(ci.SCALES)


def _sum_bound(k_terms, ws_sum=1):
    return ((k_terms + 2) + (ws_sum - 1)) * U


def _build(engine, dev, pdt, comm=None, shapes=SHAPES, groups=None, **kw):
    """(model, params, optimizer) of ZeRO-``engine`` over probes of ``shapes``."""
    from zero_amd import zero3

    init = z3c._init_weights(pdt, shapes)
    tdt = torch.float32 if pdt == "f32" else BF16
    model = ProbeModel([Probe(torch.from_numpy(w.copy()).to(dev, tdt)) for w in init])
    params = [m.weight for m in model.probes]
    if groups is None:
        inner = torch.optim.Adam(params, **z3c.ADAM)
    else:
        inner = torch.optim.AdamW([dict(params=[params[i] for i in idx], **g) for idx, g in groups])
    if comm is not None:
        kw["comm"] = comm
    if engine == 3:
        opt = zero3.ShardedOptimizer(inner, update=True, bucket_mb=z3c.BUCKET_MB, **kw)
        zero3.register_zero3_hooks(model, opt.param_managers)
    else:
        opt = module_for(engine).ShardedOptimizer(inner, **kw)
    return model, params, opt


def _backward(engine, model, opt, step, rank, pdt, dev, shapes=SHAPES, on=None, nan_in=None):
    if engine != 3:
        opt.zero_grad()
    for k, m in enumerate(model.probes):
        c = ci.local(step, 0, rank, k, pdt, shapes).copy()
        if nan_in == k:
            c.reshape(-1)[c.size // 2] = np.nan
        m.c = torch.from_numpy(c).to(dev, m.weight.dtype)
    model([True] * len(shapes) if on is None else on).backward()


def _held(engine, opt, i):
    """Whether this rank holds (a share of) parameter i's master."""
    return engine == 3 or i in opt.local_param_indices


def _masters(engine, opt, params):
    """This rank's share of every parameter's fp32 master, flat float32 (None: holds none)."""
    from zero_amd._update import join_split_master

    torch.cuda.synchronize()
    out = []
    for i, p in enumerate(params):
        if not _held(engine, opt, i):
            out.append(None)
            continue
        st = opt.optimizer.state[p] if p in opt.optimizer.state else {}
        if p.dtype == torch.float32:
            m = p.detach()
        elif st.get("master_param") is not None:
            m = st["master_param"]
        elif st.get("master_residual") is not None:
            m = join_split_master(p, st["master_residual"])
        else:  # (no residual yet: the master is the parameter)
            m = p.detach().float()
        out.append(m.detach().float().cpu().numpy().reshape(-1).copy())
    return out


def _sums(before, after, ws):
    """Per parameter (sum d^2, sum after^2) in float64, over all ranks' shares."""
    local = []
    for b, a in zip(before, after):
        if a is None:
            local.append((0.0, 0.0))
            continue
        d = (a - b).astype(np.float32)
        local.append((float((d.astype(np.float64) ** 2).sum()), float((a.astype(np.float64) ** 2).sum())))
    if ws == 1:
        return local
    every = [None] * ws
    dist.all_gather_object(every, local)
    return [tuple(sum(r[i][k] for r in every) for k in (0, 1)) for i in range(len(local))]


class _Watch:
    """The two vectors of ``opt`` over its steps: the same tensors every step, NaN before the first,
    every entry in bound, +0.0 / kept where nothing was measured, the same bits on every rank."""

    def __init__(self, opt, n, ws=1):
        self.opt, self.n, self.ws = opt, n, ws
        self.un, self.wn = opt.last_param_update_norms, opt.last_param_weight_norms
        for t in (self.un, self.wn):
            assert t.dim() == 1 and t.dtype == torch.float32 and t.numel() == n and t.is_cuda
            assert torch.isnan(t).all(), "not measured yet"
        self.prev_w = self.wn.cpu().numpy().copy()

    def check(self, sums, updated, bound, what):
        opt = self.opt
        assert opt.last_param_update_norms is self.un and opt.last_param_weight_norms is self.wn
        torch.cuda.synchronize()
        un, wn = self.un.cpu().numpy(), self.wn.cpu().numpy()
        worst = 0.0
        for i in range(self.n):
            if not updated[i]:
                assert un[i].view(np.uint32) == 0, f"{what} param {i}: update {un[i]!r}, not +0.0"
                assert wn[i].view(np.uint32) == self.prev_w[i].view(np.uint32), f"{what} param {i}"
                continue
            for got, want in ((un[i], sums[i][0]), (wn[i], sums[i][1])):
                assert np.isfinite(got) and want > 0, (what, i, got, want)
                rel = abs(float(got) - np.sqrt(want)) / np.sqrt(want)
                worst = max(worst, rel / (bound / 2 + U))
                assert rel <= bound / 2 + U, (what, i, rel, bound / 2 + U)
        print(f"{what}: worst norm error {worst:.3f} of its bound")
        if self.ws > 1:
            every = [None] * self.ws
            dist.all_gather_object(every, (un.view(np.uint32).tolist(), wn.view(np.uint32).tolist()))
            assert all(e == every[0] for e in every), "the ranks report different bits"
        self.prev_w = wn.copy()


def _run(engine, gpu, pdt, k_terms, steps=STEPS, off_at=None, nan_at=None, rank=0, ws=1, comm=None,
         shapes=SHAPES, frozen=None, ws_sum=1, **kw):
    """``steps`` probe steps with every check; returns (params, opt, model).  ``off_at`` =
    (step, parameter): no gradient for it in that step; ``nan_at`` likewise plants a NaN."""
    model, params, opt = _build(engine, gpu, pdt, comm, shapes, param_update_norms=True, **kw)
    watch = _Watch(opt, len(params), ws)
    bound = _sum_bound(k_terms, ws_sum)
    for t in range(steps):
        on = [i != frozen and (off_at is None or off_at != (t, i)) for i in range(len(shapes))]
        nan_in = nan_at[1] if nan_at is not None and nan_at[0] == t else None
        before = _masters(engine, opt, params)  # (backward does not touch the master)
        _backward(engine, model, opt, t, rank, pdt, gpu, shapes, on, nan_in)
        if t == 0 and opt.max_grad_norm is not None:
            g = [ci.values(ci.reduced(0, 0, i, list(range(ws)), pdt, shapes)) for i in range(len(shapes))
                 if i != frozen]
            opt.max_grad_norm = 4.0 * float(np.sqrt(sum((x ** 2).sum() for x in g))) / ws
        opt.step()
        after = _masters(engine, opt, params)
        skipped = nan_in is not None
        if skipped:
            assert int(opt.skipped_steps.item()) == 1 and np.isnan(opt.last_clip_coef.item())
            for b, a in zip(before, after):
                assert a is None or np.array_equal(b.view(np.uint32), a.view(np.uint32))
        watch.check(_sums(before, after, ws), [o and not skipped for o in on], bound,
                    f"ZeRO-{engine} {pdt} rank {rank} step {t}")
    return params, opt, model


# ---------------------------------------------------------------------------------------------
# world size 1
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [1, 2, 3])
def test_ws1_fp32_two_groups(gpu, pg1, engine):
    """fp32 parameters in two AdamW groups; parameter 1 has no gradient in the second step."""
    _run(engine, gpu, "f32", 8, groups=GROUPS, off_at=(1, 1))


@pytest.mark.parametrize("engine", [1, 2, 3])
def test_ws1_bf16_split_clipped_with_grad_norms(gpu, pg1, engine):
    """bf16 parameters over the split master through a real backward, with clipping (the second
    step is clipped to about 0.1) and ``param_grad_norms`` beside it."""
    _, opt, _ = _run(engine, gpu, "bf16", 16, max_grad_norm=1.0, param_grad_norms=True, off_at=(2, 0))
    assert opt.last_param_grad_norms is not None and opt.last_param_grad_norms.numel() == len(SHAPES)
    assert float(opt.last_clip_coef.item()) == 1.0


def test_ws1_bf16_fp32_master(gpu, pg1):
    _run(2, gpu, "bf16", 8, master="fp32")


@pytest.mark.parametrize("engine", [2, 3])
@pytest.mark.parametrize("pdt", ["f32", "bf16"])
def test_ws1_a_skipped_step_measures_nothing(gpu, pg1, engine, pdt):
    """``skip_nonfinite``: the second step carries a NaN and is skipped -- every update norm +0.0,
    every weight norm the first step's -- and the third measures again."""
    _run(engine, gpu, pdt, 16 if pdt == "bf16" else 8, max_grad_norm=1.0, skip_nonfinite=True,
         nan_at=(1, 1))


def _raw(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().copy()


@pytest.mark.parametrize("engine", [2, 3])
def test_switch_off(gpu, pg1, engine):
    """Without the option the attributes are None, no stage exists, and parameters and state have
    the bits of the run with it: the measurement does not enter the trajectory."""
    runs = []
    for on in (False, True):
        model, params, opt = _build(engine, gpu, "bf16", param_update_norms=on)
        for t in range(2):
            _backward(engine, model, opt, t, 0, "bf16", gpu)
            opt.step()
        torch.cuda.synchronize()
        runs.append((params, opt))
    (p0, o0), (p1, o1) = runs
    assert o0.last_param_update_norms is None and o0.last_param_weight_norms is None
    assert (o0._stats if engine == 3 else o0.engine.stats) is None
    assert o1.last_param_update_norms is not None
    for a, b in zip(p0, p1):
        assert np.array_equal(_raw(a), _raw(b))
        for name in ("exp_avg", "exp_avg_sq", "master_residual"):
            assert np.array_equal(_raw(o0.optimizer.state[a][name]), _raw(o1.optimizer.state[b][name])), name


def test_refusals(gpu, pg1):
    """On the device as on the host (tests/test_update_norms_host.py), and at the step where a
    group turns amsgrad on."""
    from zero_amd import zero1, zero2, zero3

    P = lambda dt=torch.float32: [torch.nn.Parameter(torch.zeros(8, device=gpu, dtype=dt))]  # noqa: E731
    for mod, kw in ((zero1, {}), (zero2, {}), (zero3, dict(update=True))):
        with pytest.raises(ValueError, match="param_update_norms.*SGD"):
            mod.ShardedOptimizer(torch.optim.SGD(P(), lr=0.1), param_update_norms=True, **kw)
        with pytest.raises(ValueError, match="param_update_norms.*amsgrad"):
            mod.ShardedOptimizer(torch.optim.Adam(P(), amsgrad=True), param_update_norms=True, **kw)
        with pytest.raises(ValueError, match="param_update_norms.*ema_decay"):
            mod.ShardedOptimizer(torch.optim.Adam(P()), param_update_norms=True, ema_decay=0.9, **kw)
        with pytest.raises(ValueError, match="param_update_norms.*master='none'"):
            mod.ShardedOptimizer(torch.optim.Adam(P(BF16)), param_update_norms=True, master="none", **kw)
        with pytest.raises(ValueError, match="param_update_norms.*bfloat16"):
            mod.ShardedOptimizer(torch.optim.Adam(P(BF16), betas=(0.9, 0.99)), param_update_norms=True,
                                 state_dtype=BF16, **kw)
        params = P()
        opt = mod.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), param_update_norms=True, **kw)
        opt.optimizer.param_groups[0]["amsgrad"] = True
        params[0].grad = torch.ones(8, device=gpu)
        with pytest.raises(ValueError, match="param_update_norms.*amsgrad"):
            opt.step()
    with pytest.raises(ValueError, match="param_update_norms.*update mode"):
        zero3.ShardedOptimizer(torch.optim.Adam(P()), update=False, param_update_norms=True)
    with pytest.raises(ValueError, match="param_update_norms.*overlap"):
        zero2.ShardedOptimizer(torch.optim.Adam(P()), overlap=True, param_update_norms=True)
    with pytest.raises(ValueError, match="param_update_norms.*bucket arena"):
        zero2.ShardedOptimizer(torch.optim.Adam(P()), arena="buckets", param_update_norms=True)


# ---------------------------------------------------------------------------------------------
# world size 2, gloo-staged
# ---------------------------------------------------------------------------------------------
def _ws2_zero2_worker(rank, ws, port, layout):
    """ZeRO-2 fp32 on the flat arena with 64-element windows: (66, 128) is cut across many rounds;
    parameter 2 never has a gradient.  Every parameter has one owner, the other rank adds 0."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    _, opt, _ = _run(2, dev, "f32", 8, rank=rank, ws=ws, comm=test_comm(), groups=GROUPS, frozen=2,
                     off_at=(1, 4), layout=layout, bucket_mb=ws * 64 * 4 / (1 << 20))
    assert layout != "reference" or opt.engine.K > 1
    dist.barrier()
    dist.destroy_process_group()


def _ws2_zero3_worker(rank, ws, port, pdt):
    """ZeRO-3 update mode on tests/_clip_inputs.py's shapes -- (7, 24) in chunks of 4 and 3 rows,
    (1,) with an empty chunk on rank 1 -- an entry being the norm over both ranks' chunks; clipped,
    with a skipped second step."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    _, opt, _ = _run(3, dev, pdt, 16 if pdt == "bf16" else 8, rank=rank, ws=ws, comm=test_comm(),
                     shapes=ci.SHAPES, ws_sum=ws, max_grad_norm=1.0, skip_nonfinite=True, nan_at=(1, 0))
    assert int(opt._arena.ln[3]) == (1 if rank == 0 else 0)
    dist.barrier()
    dist.destroy_process_group()


def _ws2_zero1_refused_worker(rank, ws, port):
    from zero_amd import zero1

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    p = torch.nn.Parameter(torch.zeros(8, device="cuda:0"))
    with pytest.raises(ValueError, match="param_update_norms.*ZeRO-1 at world size > 1"):
        zero1.ShardedOptimizer(torch.optim.Adam([p], lr=1e-3), param_update_norms=True)
    dist.destroy_process_group()


def test_ws2_gloo(gpu):
    spawn_batch(2, [(_ws2_zero2_worker, ("reference",)), (_ws2_zero2_worker, ("flat",)),
                    (_ws2_zero3_worker, ("f32",)), (_ws2_zero3_worker, ("bf16",)),
                    (_ws2_zero1_refused_worker, ())])
