"""``zero3.ShardedOptimizer(update=True, ema_decay=d)``: the EMA of this rank's chunks equals
tests/_ema_oracle.py composed over the oracle's own trajectory, bit for bit, at world size 1 and 2.

Probe modules (tests/test_gpu_zero3_accumulate.py) make every gradient a planted tensor: integers in
[-40, 40] times 2^-12, distinct per rank, pass, step and parameter, so the sum over the ranks and
passes is exact in bf16 and in fp32 and the update's gradient is known exactly.  Every rank follows
the oracle of every rank's rows, so inside ``ema_parameters()`` a forward is compared with the
forward of a plain copy of the model that holds the expected full weights.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _clip_inputs as ci
import _ema_oracle as eo
from _zero_run import init_pg, spawn_batch
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_clip_optimizer import pg1, rccl_env  # noqa: F401
from test_gpu_ema_optimizer import _same, host
from test_gpu_zero3_accumulate import Probe, ProbeModel, _rows
from test_gpu_zero3_clip import ADAM, HP, _build

pytestmark = pytest.mark.gpu

SHAPES = ci.SHAPES  # (66, 128), (7, 24), (16,), (1,): at ws = 2 the last one leaves rank 1 no rows
DECAYS = (0.999, 0.999, 0.9, 0.9, 0.9)  # changed before the third step


def _local(step, pas, rank, i):
    rng = np.random.default_rng([23, step, pas, rank, i])
    return (rng.integers(-40, 41, SHAPES[i]) * 2.0 ** -12).astype(np.float32)


def _total(step, passes, ws, i):
    """The exact sum over ranks and passes (fp32; a bf16 arena holds the same values)."""
    s = sum(_local(step, pas, r, i).astype(np.float64) for pas in range(passes) for r in range(ws))
    s = s.astype(np.float32)
    assert np.array_equal(zo.bf16_bits_to_f32(zo.f32_to_bf16_bits(s)), s)
    return s


class _Ref:
    """One rank's rows of one parameter: the split master (bf16) or fp32 parameters."""

    def __init__(self, rows, pdt):
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1)
        self.split, self.t, n = pdt == "bf16", 0, rows.size
        self.m, self.v, self.ema = np.zeros(n, np.float32), np.zeros(n, np.float32), rows.copy()
        if self.split:
            self.hi, self.lo = zo.f32_to_bf16_bits(rows), np.zeros(n, np.uint16)
        else:
            self.p = rows.copy()

    def step(self, gsum, div, decay, coef=None):
        self.t += 1
        hp = c_oracle.hparams(step=self.t, **HP)
        g = eo.prep(gsum, div, coef)
        if self.split:
            eo.adam_ema_split(self.hi, self.lo, g, self.m, self.v, self.ema, hp, decay)
        else:
            eo.adam_ema_f32(self.p, g, self.m, self.v, self.ema, hp, decay)

    def ema_as_param(self):
        return zo.f32_to_bf16_bits(self.ema) if self.split else self.ema

    def check(self, p, st, what):
        _same(host(p), self.hi if self.split else self.p, what + " param")
        _same(host(st["exp_avg"]), self.m, what + " exp_avg")
        _same(host(st["exp_avg_sq"]), self.v, what + " exp_avg_sq")
        _same(host(st["ema_param"]), self.ema, what + " ema_param")
        assert st["ema_param"].shape == p.shape and st["ema_param"].dtype == torch.float32
        if self.split:
            _same(host(st["master_residual"]), self.lo, what + " residual")


def _backward(model, step, pas, rank, dev, bad=None):
    for k, m in enumerate(model.probes):
        c = _local(step, pas, rank, k)
        if bad is not None and k == bad[0]:
            c.reshape(-1)[bad[1]] = np.inf
        m.c = torch.from_numpy(c).to(dev, m.weight.dtype)
    model([True] * len(SHAPES)).backward()


def _refs(init, pdt, ws):
    return [[_Ref(_rows(w, SHAPES[i], ws, r), pdt) for i, w in enumerate(init)] for r in range(ws)]


def _step(model, params, opt, refs, step, rank, ws, dev, what, passes=1, clip=False, bad=None):
    """One step on the device and on every rank's oracle; ``bad``: (parameter, flat index) of an
    inf planted in rank ws - 1's gradient, the step is then skipped."""
    ar = opt._arena
    for pas in range(passes):
        _backward(model, step, pas, rank, dev, bad if rank == ws - 1 else None)
    opt.step()
    torch.cuda.synchronize()
    coef = np.float32(opt.last_clip_coef.item()) if clip else None
    if bad is not None:
        assert np.isnan(coef)
    elif clip:
        assert 0 < coef < 1, coef
    for r in range(ws):
        for i, ref in enumerate(refs[r]):
            if ref.m.size == 0:
                continue
            if bad is not None:
                ref.t += 1  # the host's count advances; nothing else does
            else:
                ref.step(_rows(_total(step, passes, ws, i), SHAPES[i], ws, r), float(ws),
                         DECAYS[step], coef)
    for i, p in enumerate(params):
        if int(ar.ln[i]):
            refs[rank][i].check(p, opt.optimizer.state[p], f"{what} step {step} param {i}")


def _trajectory(rank, ws, dev, comm, pdt, passes=1, acc32=False, clip=False):
    kw = dict(ema_decay=DECAYS[0])
    if passes > 1:
        kw.update(grad_accumulation=True, accumulation_dtype=torch.float32 if acc32 else None)
    if clip:
        kw.update(max_grad_norm=1e-2, skip_nonfinite=True, param_grad_norms=True)
    model, params, opt, init = _build(dev, pdt, comm, SHAPES, **kw)
    ar, refs = opt._arena, _refs(init, pdt, ws)
    what = f"zero3 ws={ws} rank {rank} {pdt} passes={passes}"
    assert opt.ema_decay == DECAYS[0] and opt._core.ema is not None
    for i, p in enumerate(params):  # the EMA starts at the master, chunk-shaped
        if int(ar.ln[i]):
            _same(host(opt.optimizer.state[p]["ema_param"]), refs[rank][i].ema, what + " initial")
    for step in range(4):
        if step == 2:
            opt.ema_decay = DECAYS[2]
            with pytest.raises(ValueError, match="ema_decay"):
                opt.ema_decay = -0.1
        # with clipping, step 2 (the second) carries an inf: the EMA of step 1 stays in place
        bad = (0, 5) if clip and step == 1 else None
        _step(model, params, opt, refs, step, rank, ws, dev, what, passes, clip, bad)
    if clip:
        assert int(opt.skipped_steps.item()) == 1
    if acc32 and ws > 1 and pdt == "bf16":
        assert opt._A is not None  # the update read the fp32 accumulation arena
    # ---- ema_parameters(): the gathers hand every rank RNE(ema) of the owners' EMA
    views = lambda i: {k: v for k, v in opt.optimizer.state[params[i]].items() if k != "step"}  # noqa: E731
    before = [(host(p), {k: host(v) for k, v in views(i).items()}) for i, p in enumerate(params)]
    tdt = torch.float32 if pdt == "f32" else torch.bfloat16
    full = []
    for i, s in enumerate(SHAPES):  # dim-0 chunks in rank order are the full tensor, flat
        flat = np.concatenate([refs[r][i].ema_as_param() for r in range(ws)])
        t = torch.from_numpy(flat.view(np.int16) if pdt == "bf16" else flat)
        full.append((t.view(torch.bfloat16) if pdt == "bf16" else t).reshape(s).to(dev))
    plain = ProbeModel([Probe(w.clone()) for w in full])
    cs = [torch.from_numpy(_local(9, 0, 0, k)).to(dev, tdt) for k in range(len(SHAPES))]
    for m, pm, c in zip(model.probes, plain.probes, cs):
        m.c = pm.c = c
    on = [True] * len(SHAPES)
    with torch.no_grad():
        want = host(plain(on))
        outside = host(model(on))
    with opt.ema_parameters():
        for i, p in enumerate(params):
            if int(ar.ln[i]):
                _same(host(p), refs[rank][i].ema_as_param(), f"{what} inside, chunk {i}")
        with torch.no_grad():
            inside = host(model(on))
        for call in (opt.step, opt.state_dict, lambda: opt.load_state_dict({}),
                     lambda: opt.ema_parameters().__enter__()):
            with pytest.raises(RuntimeError, match="ema_parameters"):
                call()
    _same(inside, want.view(np.uint16 if pdt == "bf16" else np.uint32), what + " forward inside")
    assert not np.array_equal(outside, want)  # (the weights themselves give another value)
    with torch.no_grad():
        _same(host(model(on)), outside, what + " forward after exit")
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        _same(host(p), before[i][0], f"{what} after exit, chunk {i}")
        for k, v in views(i).items():
            _same(host(v), before[i][1][k], f"{what} after exit, {k} of param {i}")
    _step(model, params, opt, refs, 4, rank, ws, dev, what + " (after the context)", passes, clip)
    return opt


def _checkpoint(rank, ws, dev, comm, pdt):
    """2 steps + save + fresh optimizer + load + 2 steps equals 4 steps, the EMA included; then the
    two loading rules."""
    model, params, opt, init = _build(dev, pdt, comm, SHAPES, ema_decay=DECAYS[0])
    refs = _refs(init, pdt, ws)
    what = f"checkpoint zero3 ws={ws} rank {rank} {pdt}"
    for step in range(2):
        _step(model, params, opt, refs, step, rank, ws, dev, what)
    sd = opt.state_dict()
    chunks = [p.detach().clone() for p in params]

    def fresh(**kw):
        m2, p2, o2, _ = _build(dev, pdt, comm, SHAPES, **kw)
        with torch.no_grad():
            for p, c in zip(p2, chunks):  # this rank's chunks, before the state
                p.data.copy_(c)
        return m2, p2, o2

    model2, params2, opt2 = fresh(ema_decay=DECAYS[2])
    opt2.load_state_dict(sd)
    for step in range(2, 4):
        _step(model2, params2, opt2, refs, step, rank, ws, dev, what + " resumed")
    # ---- a dict without ema_param: that EMA starts from the loaded master
    lean = dict(sd, state={k: {n: v for n, v in e.items() if n != "ema_param"}
                           for k, e in sd["state"].items()})
    _, params3, opt3 = fresh(ema_decay=0.5)
    opt3.load_state_dict(lean)
    torch.cuda.synchronize()
    for i, p in enumerate(params3):
        if int(opt3._arena.ln[i]) == 0:
            continue
        st, e = opt3.optimizer.state[p], sd["state"][i]
        want = c_oracle.join_master(host(chunks[i]), host(e["master_residual"])) if pdt == "bf16" \
            else host(chunks[i])
        _same(host(st["ema_param"]), want, f"{what} lean load, param {i}")
    # ---- entries with ema_param into an optimizer without ema_decay: refused
    _, _, opt4 = fresh()
    assert opt4.ema_decay is None and opt4._core.ema is None
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
    globals()[fn](rank, ws, torch.device("cuda:0"), test_comm(), *args)
    dist.barrier()
    dist.destroy_process_group()
    if rank:
        faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("pdt,passes,acc32,clip", [("bf16", 1, False, False), ("f32", 1, False, False),
                                                   ("bf16", 2, True, False), ("bf16", 1, False, True)],
                         ids=["split", "f32", "split-accumulate-fp32", "split-clip-skip"])
def test_ws1_trajectory(gpu, pg1, pdt, passes, acc32, clip):
    from _gloo_comm import test_comm

    _trajectory(0, 1, gpu, test_comm(), pdt, passes, acc32, clip)


@pytest.mark.parametrize("pdt", ["bf16", "f32"])
def test_ws1_checkpoint(gpu, pg1, pdt):
    from _gloo_comm import test_comm

    _checkpoint(0, 1, gpu, test_comm(), pdt)


def test_ws2(gpu):
    spawn_batch(2, [(_mr, ("_trajectory", "bf16")),
                    (_mr, ("_trajectory", "f32")),
                    (_mr, ("_trajectory", "bf16", 2, True)),
                    (_mr, ("_trajectory", "bf16", 1, False, True)),
                    (_mr, ("_checkpoint", "bf16"))])


def test_ws2_rccl(gpu, rccl_env):
    spawn_batch(2, [(_mr, ("_trajectory", "bf16", 2, True))], all_spawned=True)
