"""``zero3.ShardedOptimizer(update=True, master="none")``: bf16 chunks without any master, at world
size 1 and as rank 0 of a simulated two-rank job (SimRankComm: the other rank contributes zeros).

Gradients are known exactly (tests/_clip_inputs.py: probe modules whose gradient is a planted
coefficient tensor).  Five steps under ``max_grad_norm`` and ``skip_nonfinite``, scaled x1, x40,
x0.05, x1 and x40 with the limit at four times the first step's norm — coefficients 1, about 0.1, 1,
(skipped), about 0.1; the fourth step carries one +Inf and must leave chunks and moments as they
are, count in ``skipped_steps`` and still consume its key.  Every other step equals the restatement
of tests/_psr_oracle.py bit for bit, fed the pre-clipped gradient with the coefficient the device
reported.  Two passes per step under ``accumulation_dtype=torch.float32`` read the fp32 arena: the
fp32-gradient instances.
"""
import numpy as np
import pytest
import torch

import _clip_inputs as ci
import _psr_oracle as po
import test_gpu_zero3_clip as zc
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_clip_optimizer import pg1  # noqa: F401
from test_gpu_zero3_accumulate import _rows
from test_gpu_zero3_clip import sim2  # noqa: F401

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SEED = zc.SEED
SHAPES = ci.SHAPES
STATE_KW = {"f32": {}, "bf16": dict(state_dtype=BF16),
            "bf16_sr": dict(state_dtype=BF16, state_rounding="stochastic")}
BYTES = {"f32": 22, "bf16": 14, "bf16_sr": 14}
STEPS = 5
BAD_STEP = 3
host, _same, _f32 = zc.host, zc._same, zc._f32


class _Ref:
    """This rank's rows of one parameter under the master-free restatement."""

    def __init__(self, rows, state, slot):
        self.p = zo.f32_to_bf16_bits(np.ascontiguousarray(rows, np.float32).reshape(-1))
        z = np.float32 if state == "f32" else np.uint16
        self.m, self.v = np.zeros(self.p.size, z), np.zeros(self.p.size, z)
        self.state, self.t = state, 0
        self.e = np.uint64(slot) + np.arange(self.p.size, dtype=np.uint64)

    def step(self, g, div, coef):
        self.t += 1
        g = np.ascontiguousarray(g).reshape(-1)
        gf = zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g
        with np.errstate(all="ignore"):
            gp = np.ascontiguousarray((gf / np.float32(div)).astype(np.float32) * np.float32(coef))
        chp = c_oracle.hparams(step=self.t, grad_div=1.0, **zc.HP)
        po.step(self.p, gp, self.m, self.v, chp, self.e, po.keys_of(SEED, self.t), self.state)

    def check(self, p, st, what):
        _same(host(p), self.p, what + " param")
        assert "master_residual" not in st and "master_param" not in st, what
        _same(host(st["exp_avg"]), self.m, what + " exp_avg")
        _same(host(st["exp_avg_sq"]), self.v, what + " exp_avg_sq")


def _case(rank, ws, dev, comm, state, passes=1, acc32=False, sim=False):
    ranks = [rank] if sim or ws == 1 else list(range(ws))
    widen = acc32 and passes >= 2 and ws > 1
    kw = dict(STATE_KW[state], master="none", state_seed=SEED, max_grad_norm=1.0,
              skip_nonfinite=True)
    if passes > 1:
        kw.update(grad_accumulation=True, accumulation_dtype=torch.float32 if acc32 else None)
    model, params, opt, init = zc._build(dev, "bf16", comm, SHAPES, **kw)
    ar, core = opt._arena, opt._core
    assert core.master_free and core.lo is None and core.master is None and not opt._split
    ref = [_Ref(_rows(w, SHAPES[i], ws, rank), state, int(ar.slot[i])) for i, w in enumerate(init)]
    coefs, skipped, before = [], 0, None
    for step in range(STEPS):
        k = step % len(ci.SCALES)  # the inputs of steps 0 to 2 again
        bad = step == BAD_STEP
        for pas in range(passes):
            for j, m in enumerate(model.probes):
                c = ci.local(k, pas, rank, j, "bf16").copy()
                if bad and pas == 0 and j == 0:
                    c[0, 5] = np.inf  # row 0: rank 0's chunk
                m.c = torch.from_numpy(c).to(dev, BF16)
            model([True] * len(SHAPES)).backward()
        grads = [ci.accumulated(k, passes, i, ranks, "bf16", widen) for i in range(len(SHAPES))]
        if step == 0:
            opt.max_grad_norm = 4.0 * zc._norm64(grads, ws, rank, sim, SHAPES)
        opt.step()
        torch.cuda.synchronize()
        what = f"rank {rank} step {step}"
        assert [int(s) for s in opt._steps] == [(step + 1) * int(n > 0) for n in ar.ln], what
        if widen:
            assert opt._fast_sets.get(True) and opt._A is not None
        if bad:
            skipped += 1
            assert np.isnan(_f32(opt.last_clip_coef)), what
            for i, p in enumerate(params):
                assert np.array_equal(host(p), before[i][0]), f"{what}: param {i} moved"
                for name, v in opt._state_views(i).items():
                    assert np.array_equal(host(v), before[i][1][name]), f"{what}: {name} {i} moved"
            for r in ref:
                r.t += 1  # the host's count advances and the step's key is spent; nothing else
        else:
            coefs.append(_f32(opt.last_clip_coef))
            per = BYTES[state] + (2 if widen else 0)
            assert core.last_adam_bytes == per * int(ar.ln.sum()), what
            for i, (p, r) in enumerate(zip(params, ref)):
                if int(ar.ln[i]):
                    r.step(_rows(grads[i], SHAPES[i], ws, rank), float(ws), coefs[-1])
                    r.check(p, opt.optimizer.state[p], f"{what} param {i}")
        assert int(opt.skipped_steps.item()) == skipped, what
        before = [(host(p), {n: host(v) for n, v in opt._state_views(i).items()})
                  for i, p in enumerate(params)]
    print("coefficients", coefs)
    assert [c.view(np.uint32) == zc.ONE for c in coefs] == [True, False, True, False]
    assert all(0.05 < coefs[j] < 0.2 for j in (1, 3))
    assert skipped == 1 and int(opt.skipped_steps.item()) == 1
    return opt


@pytest.mark.parametrize("state", list(STATE_KW))
def test_ws1(gpu, pg1, state):
    _case(0, 1, gpu, None, state)


@pytest.mark.parametrize("state", list(STATE_KW))
def test_simulated_rank(gpu, sim2, state):
    from _gloo_comm import SimRankComm

    _case(sim2, 2, gpu, SimRankComm(2, sim2), state, sim=True)


@pytest.mark.parametrize("state", ["f32", "bf16_sr"])
def test_simulated_rank_fp32_accumulation(gpu, sim2, state):
    """Two passes under accumulation_dtype=torch.float32: the update reads the fp32 arena."""
    from _gloo_comm import SimRankComm

    opt = _case(0, 2, gpu, SimRankComm(2, 0), state, passes=2, acc32=True, sim=True)
    assert opt._A is not None and opt._A.dtype == torch.float32


def test_refusals_and_checkpoints(gpu, pg1):
    from zero_amd import zero3

    P = lambda dt=BF16: [torch.nn.Parameter(torch.zeros(8, 4, dtype=dt, device=gpu))]  # noqa: E731
    mk = lambda params, **kw: zero3.ShardedOptimizer(  # noqa: E731
        torch.optim.Adam(params, lr=1e-3, **kw.pop("adam", {})), **kw)
    with pytest.raises(ValueError, match="update mode"):
        mk(P(), update=False, master="none")
    with pytest.raises(ValueError, match="bf16 parameters"):
        mk(P(torch.float32), update=True, master="none")
    with pytest.raises(ValueError, match="amsgrad"):
        mk(P(), update=True, master="none", adam=dict(amsgrad=True))
    with pytest.raises(ValueError, match="SGD"):
        zero3.ShardedOptimizer(torch.optim.SGD(P(), lr=0.1), update=True, master="none")
    with pytest.raises(ValueError, match="master must be"):
        mk(P(), update=True, master="fp32")
    with pytest.raises(ValueError, match="state_seed"):
        mk(P(), update=True, master="none", state_seed=-1)

    def stepped(master, seed):
        params = P()
        opt = mk(params, update=True, master=master, state_seed=seed)
        params[0].grad = torch.full_like(params[0], 0.25)
        opt.step()
        torch.cuda.synchronize()
        return params, opt

    ps, osplit = stepped("split", 0)
    pn, onone = stepped("none", 7)
    sd_split, sd_none = osplit.state_dict(), onone.state_dict()
    assert sd_split["zero_amd"]["master"] == "split" and "state_seed" not in sd_split["zero_amd"]
    assert sd_none["zero_amd"]["master"] == "none" and sd_none["zero_amd"]["state_seed"] == 7
    assert sorted(sd_none["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert sorted(onone.optimizer.state[pn[0]]) == ["exp_avg", "exp_avg_sq", "step"]
    with pytest.raises(ValueError, match="master_residual"):
        onone.load_state_dict(sd_split)
    osplit.load_state_dict(sd_none)  # the other way round loads: the residual starts at 0
    assert not osplit.optimizer.state[ps[0]]["master_residual"].any()
    other = mk(P(), update=True, master="none", state_seed=1)
    other.load_state_dict(sd_none)
    assert other.state_seed == other._core.state_seed == 7
    # amsgrad switched on between steps is refused at the step
    onone.optimizer.param_groups[0]["amsgrad"] = True
    pn[0].grad = torch.full_like(pn[0], 0.25)
    with pytest.raises(ValueError, match="amsgrad"):
        onone.step()
