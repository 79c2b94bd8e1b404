"""``ShardedOptimizer(..., ema_decay=d)`` on ZeRO-1/2 (the flat arena): every owner's ``ema_param``
equals tests/_ema_oracle.py composed over the oracle's own trajectory, bit for bit.

Gradients are integers in [-40, 40] times 2^-12, distinct per rank, step and parameter: a sum over
up to three ranks is exact in bf16 and in fp32 under any order, so the reduced gradient is known
exactly at every world size.  Four steps of AdamW with the decay changed before the third; then
``ema_parameters()`` (every rank's parameters are the owners' EMA rounded to nearest even, restored
bit for bit on exit, ``step()`` refused inside), a fifth step that continues the uninterrupted
trajectory, and the checkpoint round trip with its two loading rules.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _ema_oracle as eo
from conftest import free_port
from _zero_run import init_pg, module_for, set_grad, spawn_batch
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_clip_optimizer import pg1, rccl_env  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(100, 90), (64,), (4096 + 40,), (7, 5)]
HP = dict(lr=1e-3, weight_decay=1e-2, decoupled=True)
DECAYS = (0.999, 0.999, 0.9, 0.9, 0.9)  # changed before the third step


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


def _init(pdt, shapes=SHAPES):
    rng = np.random.default_rng(5)
    out = []
    for s in shapes:
        w = (rng.standard_normal(s) * 0.1).astype(np.float32)
        if pdt == "bf16":
            w = zo.bf16_bits_to_f32(zo.f32_to_bf16_bits(w)).reshape(s)
        out.append(w)
    return out


def _local(step, rank, i, shape):
    rng = np.random.default_rng([17, step, rank, i])
    return (rng.integers(-40, 41, shape) * 2.0 ** -12).astype(np.float32)


def _reduced(step, ws, i, shape, pdt):
    """The exact sum over the ranks, as the update reads it: fp32, or bf16 codes."""
    s = sum(_local(step, r, i, shape).astype(np.float64) for r in range(ws)).astype(np.float32)
    bits = zo.f32_to_bf16_bits(s)
    assert np.array_equal(zo.bf16_bits_to_f32(bits).reshape(-1), s.reshape(-1))  # exact in bf16
    return bits.reshape(-1) if pdt == "bf16" else s.reshape(-1)


class _Ref:
    """One whole parameter under the oracle: fp32, fp32 master + bf16 parameter, or split."""

    def __init__(self, w, pdt, master):
        w = np.ascontiguousarray(w, np.float32).reshape(-1)
        self.kind = "f32" if pdt == "f32" else master
        self.t, n = 0, w.size
        self.m, self.v, self.ema = np.zeros(n, np.float32), np.zeros(n, np.float32), w.copy()
        if self.kind == "split":
            self.hi, self.lo = zo.f32_to_bf16_bits(w), np.zeros(n, np.uint16)
        else:
            self.p = w.copy()
            self.pb = zo.f32_to_bf16_bits(w)

    def step(self, gsum, div, decay, coef=None):
        self.t += 1
        hp = c_oracle.hparams(step=self.t, **HP)
        g = eo.prep(gsum, div, coef)
        if self.kind == "split":
            eo.adam_ema_split(self.hi, self.lo, g, self.m, self.v, self.ema, hp, decay)
        elif self.kind == "fp32":
            eo.adam_ema_master(self.p, self.pb, g, self.m, self.v, self.ema, hp, decay)
        else:
            eo.adam_ema_f32(self.p, g, self.m, self.v, self.ema, hp, decay)

    def param_bits(self):
        return self.hi if self.kind == "split" else self.pb if self.kind == "fp32" else self.p

    def ema_as_param(self):
        """RNE(ema) in the parameter dtype."""
        return self.ema if self.kind == "f32" else zo.f32_to_bf16_bits(self.ema)

    def check(self, p, st, owned, what):
        _same(host(p), self.param_bits(), what + " param")
        if not owned:
            return
        _same(host(st["exp_avg"]), self.m, what + " exp_avg")
        _same(host(st["exp_avg_sq"]), self.v, what + " exp_avg_sq")
        _same(host(st["ema_param"]), self.ema, what + " ema_param")
        assert st["ema_param"].shape == p.shape and st["ema_param"].dtype == torch.float32
        if self.kind == "split":
            _same(host(st["master_residual"]), self.lo, what + " residual")
        elif self.kind == "fp32":
            _same(host(st["master_param"]), self.p, what + " master")


def _params(dev, pdt, weights):
    tdt = torch.float32 if pdt == "f32" else torch.bfloat16
    return [torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(w)).to(dev, tdt)) for w in weights]


def _make(variant, params, ws, comm, pdt, master, **kw):
    es = 4 if pdt == "f32" else 2
    if comm is not None and ws > 1:
        kw["comm"] = comm
    return module_for(variant).ShardedOptimizer(
        torch.optim.AdamW(params, lr=HP["lr"], weight_decay=HP["weight_decay"]),
        bucket_mb=ws * 64 * es / (1 << 20), master=master, **kw)  # 64-element windows: many rounds


def _one_step(opt, params, refs, step, rank, ws, dev, pdt, clip, what, check_state=True):
    opt.zero_grad()
    for i, p in enumerate(params):
        set_grad(p, torch.from_numpy(_local(step, rank, i, SHAPES[i])).to(dev, p.dtype))
    opt.step()
    torch.cuda.synchronize()
    coef = None
    if clip:
        coef = np.float32(opt.last_clip_coef.item())
        assert 0 < coef < 1, coef
    for i, (p, r) in enumerate(zip(params, refs)):
        r.step(_reduced(step, ws, i, SHAPES[i], pdt), float(ws), DECAYS[step], coef)
        owned = check_state and i in opt.local_param_indices
        r.check(p, opt.optimizer.state[p] if owned else None, owned, f"{what} step {step} param {i}")


def _trajectory(rank, ws, dev, comm, variant, pdt, master="split", clip=False, layout="reference"):
    """Four steps, ema_parameters(), a fifth step."""
    kw = dict(max_grad_norm=1e-2, skip_nonfinite=True, param_grad_norms=True) if clip else {}
    if layout != "reference":
        kw["layout"] = layout
    weights = _init(pdt)
    params = _params(dev, pdt, weights)
    refs = [_Ref(w, pdt, master) for w in weights]
    opt = _make(variant, params, ws, comm, pdt, master, ema_decay=DECAYS[0], **kw)
    whole = layout == "reference"  # (Layout F cuts parameters across owners: no per-parameter views)
    what = f"zero{variant} ws={ws} rank {rank} {pdt}/{master}"
    assert opt.ema_decay == DECAYS[0] and opt.engine.ema is not None
    if whole:
        for i in opt.local_param_indices:  # the EMA starts at the master
            _same(host(opt.optimizer.state[params[i]]["ema_param"]), refs[i].ema, what + " initial")
    for step in range(4):
        if step == 2:
            opt.ema_decay = DECAYS[2]
            with pytest.raises(ValueError, match="ema_decay"):
                opt.ema_decay = 1.5
            with pytest.raises(ValueError, match="construction"):
                opt.ema_decay = None
            assert opt.ema_decay == DECAYS[2]
        _one_step(opt, params, refs, step, rank, ws, dev, pdt, clip, what, check_state=whole)
    assert not any(np.array_equal(r.ema, w.reshape(-1)) for r, w in zip(refs, weights))
    # ---- ema_parameters(): collective; every rank's parameters are RNE(ema) of the owners' EMA
    views = lambda i: {k: v for k, v in opt.optimizer.state[params[i]].items() if k != "step"}  # noqa: E731
    before = [(host(p), {k: host(v) for k, v in views(i).items()}) for i, p in enumerate(params)]
    with opt.ema_parameters():
        torch.cuda.synchronize()
        for i, (p, r) in enumerate(zip(params, refs)):
            _same(host(p), r.ema_as_param(), f"{what} inside, param {i}")
        for call in (opt.step, opt.state_dict, lambda: opt.load_state_dict({}),
                     lambda: opt.ema_parameters().__enter__()):
            with pytest.raises(RuntimeError, match="ema_parameters"):
                call()
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        _same(host(p), before[i][0], f"{what} after exit, param {i}")
        for k, v in views(i).items():
            _same(host(v), before[i][1][k], f"{what} after exit, {k} of param {i}")
    _one_step(opt, params, refs, 4, rank, ws, dev, pdt, clip, what + " (after the context)",
              check_state=whole)
    return opt


def _checkpoint(rank, ws, dev, comm, variant, pdt, master="split"):
    """2 steps + save + fresh optimizer + load + 2 steps equals 4 steps, the EMA included; then the
    two loading rules."""
    weights = _init(pdt)
    params = _params(dev, pdt, weights)
    refs = [_Ref(w, pdt, master) for w in weights]
    opt = _make(variant, params, ws, comm, pdt, master, ema_decay=DECAYS[0])
    what = f"checkpoint zero{variant} ws={ws} rank {rank} {pdt}/{master}"
    for step in range(2):
        _one_step(opt, params, refs, step, rank, ws, dev, pdt, False, what)
    sd = opt.state_dict()
    for k, e in sd["state"].items():
        assert e["ema_param"].dtype == torch.float32, k
    assert "ema_decay" not in str(sd["zero_amd"])  # the decay is a constructor argument
    saved = [p.detach().clone() for p in params]
    params2 = [torch.nn.Parameter(t.clone()) for t in saved]
    opt2 = _make(variant, params2, ws, comm, pdt, master, ema_decay=DECAYS[2])
    opt2.load_state_dict(sd)
    for step in range(2, 4):
        _one_step(opt2, params2, refs, step, rank, ws, dev, pdt, False, what + " resumed")
    # ---- a dict without ema_param: that EMA starts from the loaded master
    lean = dict(sd, state={k: {n: v for n, v in e.items() if n != "ema_param"}
                           for k, e in sd["state"].items()})
    params3 = [torch.nn.Parameter(t.clone()) for t in saved]
    opt3 = _make(variant, params3, ws, comm, pdt, master, ema_decay=0.5)
    opt3.load_state_dict(lean)
    torch.cuda.synchronize()
    index = {id(p): k for k, p in enumerate(q for g in opt3.optimizer.param_groups for q in g["params"])}
    for i in opt3.local_param_indices:
        st, e = opt3.optimizer.state[params3[i]], sd["state"][index[id(params3[i])]]
        if pdt == "f32":
            want = host(saved[i])
        elif master == "fp32":
            want = host(e["master_param"])
        else:
            want = c_oracle.join_master(host(saved[i]), host(e["master_residual"]))
        _same(host(st["ema_param"]), want, f"{what} lean load, param {i}")
        _same(host(st["exp_avg"]), host(e["exp_avg"]), f"{what} lean load exp_avg {i}")
    # ---- entries with ema_param into an optimizer without ema_decay: refused
    params4 = [torch.nn.Parameter(t.clone()) for t in saved]
    opt4 = _make(variant, params4, ws, comm, pdt, master)
    assert opt4.ema_decay is None and opt4.engine.ema is None
    if sd["state"]:
        with pytest.raises(ValueError, match="ema_param"):
            opt4.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt4.ema_parameters().__enter__()


def _mr(rank, ws, port, fn, *args):
    import faulthandler
    import sys

    from _gloo_comm import test_comm

    if rank:
        faulthandler.dump_traceback_later(120, exit=True, file=sys.stderr)
    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    globals()[fn](rank, ws, torch.device("cuda:0"), test_comm() if ws > 1 else None, *args)
    dist.barrier()
    dist.destroy_process_group()
    if rank:
        faulthandler.cancel_dump_traceback_later()


# ---- world size 1 -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,pdt,master,clip", [
    (2, "bf16", "split", False), (2, "f32", "split", False), (1, "bf16", "split", False),
    (1, "f32", "split", False), (2, "bf16", "fp32", False), (2, "bf16", "split", True),
    (2, "f32", "split", True)],
    ids=["zero2-split", "zero2-f32", "zero1-split", "zero1-f32", "zero2-fp32master",
         "zero2-split-clip-guard-norms", "zero2-f32-clip-guard-norms"])
def test_ws1_trajectory(gpu, pg1, variant, pdt, master, clip):
    opt = _trajectory(0, 1, gpu, None, variant, pdt, master, clip)
    if clip:
        assert int(opt.skipped_steps.item()) == 0 and opt.last_param_grad_norms.numel() == len(SHAPES)


def test_ws1_skipped_step_keeps_the_ema(gpu, pg1):
    """skip_nonfinite: an inf gradient in step 2 leaves every array, the EMA included, as step 1
    left it; step 3 continues from there with the host's count of 3."""
    pdt, master = "bf16", "split"
    weights = _init(pdt)
    params = _params(gpu, pdt, weights)
    refs = [_Ref(w, pdt, master) for w in weights]
    opt = _make(2, params, 1, None, pdt, master, ema_decay=0.99, max_grad_norm=float("inf"),
                skip_nonfinite=True)
    for step in range(3):
        opt.zero_grad()
        for i, p in enumerate(params):
            g = _local(step, 0, i, SHAPES[i])
            if step == 1 and i == 2:
                g[11] = np.inf
            p.grad = torch.from_numpy(g).to(gpu, p.dtype)
        opt.step()
        torch.cuda.synchronize()
        for i, (p, r) in enumerate(zip(params, refs)):
            if step == 1:
                r.t += 1  # the host's count advances; nothing else does
            else:
                r.step(_reduced(step, 1, i, SHAPES[i], pdt), 1.0, 0.99, np.float32(1.0))
            r.check(p, opt.optimizer.state[p], True, f"skip: step {step} param {i}")
    assert int(opt.skipped_steps.item()) == 1


def test_ws1_no_gradient_keeps_the_ema(gpu, pg1):
    """A parameter Adam skips for lack of a gradient keeps its EMA (and everything else)."""
    pdt, master = "f32", "split"
    weights = _init(pdt)
    params = _params(gpu, pdt, weights)
    refs = [_Ref(w, pdt, master) for w in weights]
    opt = _make(2, params, 1, None, pdt, master, ema_decay=0.9)
    for step in range(3):
        opt.zero_grad()
        for i, p in enumerate(params):
            if not (step == 1 and i == 1):
                p.grad = torch.from_numpy(_local(step, 0, i, SHAPES[i])).to(gpu)
        opt.step()
        torch.cuda.synchronize()
        for i, (p, r) in enumerate(zip(params, refs)):
            if not (step == 1 and i == 1):
                r.step(_reduced(step, 1, i, SHAPES[i], pdt), 1.0, 0.9)
            r.check(p, opt.optimizer.state[p], True, f"no grad: step {step} param {i}")


@pytest.mark.parametrize("variant,pdt,master", [(2, "bf16", "split"), (2, "f32", "split"),
                                                (1, "bf16", "fp32")],
                         ids=["zero2-split", "zero2-f32", "zero1-fp32master"])
def test_ws1_checkpoint(gpu, pg1, variant, pdt, master):
    _checkpoint(0, 1, gpu, None, variant, pdt, master)


def test_ws1_refusals_where_a_group_can_change(gpu, pg1):
    """amsgrad switched on after construction, and a decay gone bad: ValueError at the step, before
    any launch."""
    params = _params(gpu, "f32", _init("f32"))
    opt = _make(2, params, 1, None, "f32", "split", ema_decay=0.9)
    for p in params:
        p.grad = torch.ones_like(p)
    opt.optimizer.param_groups[0]["amsgrad"] = True
    before = [host(p) for p in params]
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    opt.optimizer.param_groups[0]["amsgrad"] = False
    opt._ema_decay = 2.0  # (past the setter's check)
    with pytest.raises(ValueError, match="ema_decay"):
        opt.step()
    torch.cuda.synchronize()
    for p, b in zip(params, before):
        _same(host(p), b, "refused step")


# ---- world sizes 2 and 3 --------------------------------------------------------------------------
def test_ws2(gpu):
    spawn_batch(2, [(_mr, ("_trajectory", 2, "bf16", "split")),
                    (_mr, ("_trajectory", 2, "f32", "split", True)),
                    (_mr, ("_trajectory", 2, "f32", "split", False, "flat")),
                    (_mr, ("_checkpoint", 2, "bf16", "split"))])


def test_ws3_uneven_ownership(gpu):
    spawn_batch(3, [(_mr, ("_trajectory", 2, "bf16", "split")),
                    (_mr, ("_trajectory", 2, "f32", "split"))])


def test_ws2_rccl(gpu, rccl_env):
    spawn_batch(2, [(_mr, ("_trajectory", 2, "bf16", "split"))], all_spawned=True)
