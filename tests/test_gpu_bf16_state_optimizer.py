"""``ShardedOptimizer(..., state_dtype=torch.bfloat16)``: bf16 Adam moments behind ZeRO-1/2/3.

Every trajectory is compared bit for bit with the restatement of tests/_bf16_state_oracle.py
(widen the stored moments, the unchanged C oracle step, round them to nearest even); clipped runs
take the coefficient the device reported and the unchanged oracle on the pre-clipped gradient, as
tests/test_gpu_clip_optimizer.py.  World size 2 runs through real RCCL in one batch.
"""
import io
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist

import _accum32_oracle as a32
import _bf16_state_oracle as bo
import test_gpu_zero3_accumulate_fp32 as z3t
from _zero_run import init_pg, set_grad, spawn_batch
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_clip_optimizer import pg1, rccl_env  # noqa: F401
from test_gpu_zero3_accumulate import Probe, ProbeModel, _rows

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
ADAM = dict(lr=1e-3, betas=(0.9, 0.95))  # an LLM setting; torch's default beta2 = 0.999 is refused
HP = dict(lr=1e-3, beta1=0.9, beta2=0.95)


def host(t):
    """The bits of a tensor, flat: uint16 for 16-bit dtypes, uint32 for fp32."""
    t = t.detach().cpu().contiguous().reshape(-1)
    if t.element_size() == 2:
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().view(np.uint32).copy()


def _same(got, want, what):
    want = np.ascontiguousarray(want).reshape(-1)
    want = want.view(np.uint32) if want.dtype == np.float32 else want
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:6]}"


class _Ref:
    """One parameter under the restatement: bf16 (split master) or fp32, moments as bf16 bits."""

    def __init__(self, init_bits_or_f32):
        a = np.ascontiguousarray(init_bits_or_f32).reshape(-1)
        self.split = a.dtype == np.uint16
        if self.split:
            self.hi, self.lo = a.copy(), np.zeros(a.size, np.uint16)
        else:
            self.p = a.astype(np.float32).copy()
        self.m, self.v = np.zeros(a.size, np.uint16), np.zeros(a.size, np.uint16)
        self.t = 0

    def step(self, g, div=1.0, coef=None, **hp):
        """``g``: bf16 bits or fp32, the gradient sum the update reads."""
        self.t += 1
        g = np.ascontiguousarray(g).reshape(-1)
        if coef is not None:  # the unchanged fp32 step on the pre-clipped gradient
            gf = zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g
            with np.errstate(all="ignore"):
                gp = np.ascontiguousarray((gf / np.float32(div)).astype(np.float32) * np.float32(coef))
            chp = c_oracle.hparams(step=self.t, grad_div=1.0, **{**HP, **hp})
            p = c_oracle.join_master(self.hi, self.lo) if self.split else self.p
            bo.adam_f32(p, gp, self.m, self.v, chp)
            if self.split:
                self.hi, self.lo = c_oracle.split_master(p)
            return
        chp = c_oracle.hparams(step=self.t, grad_div=float(div), **{**HP, **hp})
        if self.split and g.dtype == np.uint16:
            bo.adam_bf16_split(self.hi, self.lo, g, self.m, self.v, chp)
        elif self.split:
            bo.adam_f32grad_split(self.hi, self.lo, g, self.m, self.v, chp)
        elif g.dtype == np.uint16:  # fp32 parameters, bf16 exchange
            bo.adam_bf16(self.p, np.zeros(g.size, np.uint16), g, self.m, self.v, chp)
        else:
            bo.adam_f32(self.p, g, self.m, self.v, chp)

    def check(self, p, st, what, rows=lambda a: a):
        """``st``: optimizer.state[p] (None: a parameter this rank does not own)."""
        _same(host(p), rows(self.hi if self.split else self.p), what + " param")
        if st is None:
            return
        assert st["exp_avg"].dtype == BF16 and st["exp_avg_sq"].dtype == BF16
        assert st["exp_avg"].shape == p.shape
        if self.split:
            _same(host(st["master_residual"]), rows(self.lo), what + " residual")
        _same(host(st["exp_avg"]), rows(self.m), what + " exp_avg")
        _same(host(st["exp_avg_sq"]), rows(self.v), what + " exp_avg_sq")


# ---------------------------------------------------------------------------------------------
# world size 1: ZeRO-2 through a real backward
# ---------------------------------------------------------------------------------------------
def _mlp(gpu, dt):
    torch.manual_seed(0)
    mk = lambda *s: torch.nn.Parameter((torch.randn(*s) * 0.1).to(dt).to(gpu))  # noqa: E731
    w1, b1, w2 = mk(96, 96), mk(96), mk(96, 7)
    assert w1.numel() == 2 * 4096 + 1024  # two chunks of 4,096 and a partial one
    x, y = torch.randn(32, 96).to(dt).to(gpu), torch.randn(32, 7).to(dt).to(gpu)
    loss = lambda: (((torch.tanh(x @ w1 + b1) @ w2) - y) ** 2).sum()  # noqa: E731
    return [w1, b1, w2], loss


def _grad_bits(p):
    return host(p.grad) if p.dtype == BF16 else host(p.grad).view(np.float32)


def _init_of(p):
    return host(p) if p.dtype == BF16 else host(p).view(np.float32)


def _words(L, split):
    """fp32 words of the flat state with bf16 moments, and with fp32 ones."""
    half, pad = (L + 1) // 2, lambda w: (w + 3) // 4 * 4  # noqa: E731
    n16 = pad(half) + half
    return (pad(n16) + half if split else n16), 2 * L + (half if split else 0)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16_split", "fp32"])
def test_ws1_zero2_through_backward(gpu, pg1, dt, clip):
    from zero_amd import zero2

    params, loss = _mlp(gpu, dt)
    ref = [_Ref(_init_of(p)) for p in params]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, **ADAM), state_dtype=BF16,
                                 max_grad_norm=1.0 if clip else None)
    assert opt.state_dtype == BF16 and opt.engine.state_dtype == BF16
    assert opt.engine.split == (dt == BF16)
    L = opt.engine.L
    n16, n32 = _words(L, opt.engine.split)
    assert opt.engine.state.numel() == n16 and opt.engine.state.dtype == torch.float32
    # half of the fp32 moments' 2 L words (plus at most a pad and a rounding), the residual as it was
    assert n32 - n16 >= L - 8
    for t in range(1, 4):
        opt.zero_grad()
        (loss() * (1.0, 40.0, 0.05)[t - 1]).backward()
        grads = [_grad_bits(p) for p in params]
        coef = None
        if clip and t == 1:
            sq = sum(float(np.sum((zo.bf16_bits_to_f32(g) if g.dtype == np.uint16 else g).astype(np.float64) ** 2))
                     for g in grads)
            opt.max_grad_norm = 4.0 * np.sqrt(sq)  # coefficients: 1, about 0.1, 1
        opt.step()
        if clip:
            coef = np.float32(opt.last_clip_coef.item())
            assert (coef == 1.0) == (t != 2) and (t != 2 or 0.05 < coef < 0.2)
        assert opt.engine.last_adam_bytes == (18 if dt == BF16 else 20) * sum(p.numel() for p in params)
        for i, (p, r, g) in enumerate(zip(params, ref, grads)):
            r.step(g, coef=coef)
            r.check(p, opt.optimizer.state[p], f"step {t} param {i}")
            assert int(opt.optimizer.state[p]["step"].item()) == t


def test_ws1_fp32_master(gpu, pg1):
    """master="fp32": an fp32 master array beside the bf16 moments, 16-byte aligned."""
    from zero_amd import zero2

    params, loss = _mlp(gpu, BF16)
    init = [zo.bf16_bits_to_f32(host(p)) for p in params]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, **ADAM), state_dtype=BF16, master="fp32")
    assert opt.engine.master.data_ptr() % 16 == 0 and opt.engine.v.data_ptr() % 16 == 0
    m, v = [np.zeros(a.size, np.uint16) for a in init], [np.zeros(a.size, np.uint16) for a in init]
    for t in range(1, 4):
        opt.zero_grad()
        loss().backward()
        grads = [host(p.grad) for p in params]
        opt.step()
        assert opt.engine.last_adam_bytes == 20 * sum(p.numel() for p in params)
        for i, p in enumerate(params):
            pb = np.zeros(init[i].size, np.uint16)
            bo.adam_bf16(init[i], pb, grads[i], m[i], v[i], c_oracle.hparams(step=t, **HP))
            st = opt.optimizer.state[p]
            _same(host(p), pb, f"step {t} param {i}")
            _same(host(st["master_param"]), init[i], f"step {t} master {i}")
            _same(host(st["exp_avg"]), m[i], f"step {t} exp_avg {i}")
            _same(host(st["exp_avg_sq"]), v[i], f"step {t} exp_avg_sq {i}")


# ---------------------------------------------------------------------------------------------
# ZeRO-3 in update mode (probe modules: the gradient of a weight is its coefficient, bit for bit)
# ---------------------------------------------------------------------------------------------
def _build3(dev, comm, **kw):
    from zero_amd import zero3

    init = z3t._init_weights("bf16")
    model = ProbeModel([Probe(torch.from_numpy(w.copy()).to(dev, BF16)) for w in init])
    params = [m.weight for m in model.probes]
    if comm is not None:
        kw["comm"] = comm
    opt = zero3.ShardedOptimizer(torch.optim.Adam(params, **{**ADAM, "lr": z3t.LR}), update=True,
                                 state_dtype=BF16, bucket_mb=z3t.BUCKET_MB, **kw)
    zero3.register_zero3_hooks(model, opt.param_managers)
    return model, params, opt, [_Ref(zo.f32_to_bf16_bits(w)) for w in init]


def _zero3_schedule(rank, ws, dev, comm, passes, **kw):
    """One step per entry of ``passes`` (backward passes in it; two or more: the fp32 arena)."""
    model, params, opt, ref = _build3(dev, comm, **kw)
    assert opt.state_dtype == BF16 and opt._core.state_dtype == BF16
    for step, npass in enumerate(passes):
        chunks = [[] for _ in params]
        for pas in range(npass):
            z3t._backward(model, step, pas, rank, dev)
            for i in range(len(params)):
                chunks[i].append(z3t.delivered(step, pas, i, ws))
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        for i, (p, r) in enumerate(zip(params, ref)):
            acc = a32.accumulate_passes(chunks[i]) if ws > 1 else \
                zo.f32_to_bf16_bits(a32.exact_sum(chunks[i]).astype(np.float32))
            r.step(acc, div=float(ws), lr=z3t.LR)
            r.check(p, opt.optimizer.state[p], f"rank {rank} step {step} param {i}",
                    rows=lambda a, i=i: _rows(a, z3t.SHAPES[i], ws, rank))
    return opt


def test_ws1_zero3_update_mode(gpu, pg1):
    opt = _zero3_schedule(0, 1, gpu, None, (1, 1, 1))
    L = opt._core.L
    assert opt._core.state.numel() == _words(L, True)[0]
    assert opt._core.last_adam_bytes == 18 * sum(p.numel() for p in opt.params)


# ---------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------
def _inject(gpu, params, t):
    for i, p in enumerate(params):
        g = torch.Generator().manual_seed(977 * t + i)
        p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(p.dtype).to(gpu)


def _make(gpu, dt, **kw):
    from zero_amd import zero2

    g0 = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter((torch.randn(s, generator=g0) * 0.1).to(dt).to(gpu))
              for s in [(70, 61), (61,), (4100,)]]
    return params, zero2.ShardedOptimizer(torch.optim.Adam(params, **ADAM), **kw)


def _run(gpu, params, opt, t0, t1):
    for t in range(t0, t1):
        opt.zero_grad()
        _inject(gpu, params, t)
        opt.step()
    torch.cuda.synchronize()


def _roundtrip(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16_split", "fp32"])
def test_checkpoint_bf16_state(gpu, pg1, dt):
    """3 steps + save + a fresh optimizer + load + 3 steps = 6 steps, bit for bit."""
    pa, oa = _make(gpu, dt, state_dtype=BF16)
    _run(gpu, pa, oa, 0, 6)
    pb, ob = _make(gpu, dt, state_dtype=BF16)
    _run(gpu, pb, ob, 0, 3)
    ck = _roundtrip({"params": [p.detach().cpu() for p in pb], "opt": ob.state_dict()})
    assert all(e["exp_avg"].dtype == BF16 and e["exp_avg_sq"].dtype == BF16
               for e in ck["opt"]["state"].values())
    pc, oc = _make(gpu, dt, state_dtype=BF16)
    with torch.no_grad():
        for p, saved in zip(pc, ck["params"]):
            p.copy_(saved)
    oc.load_state_dict(ck["opt"])
    _run(gpu, pc, oc, 3, 6)
    for i, (a, c) in enumerate(zip(pa, pc)):
        _same(host(c), host(a), f"param {i}")
        for name in ("exp_avg", "exp_avg_sq") + (("master_residual",) if dt == BF16 else ()):
            _same(host(oc.optimizer.state[c][name]), host(oa.optimizer.state[a][name]), f"{name} {i}")


def test_checkpoint_fp32_to_bf16_and_back(gpu, pg1):
    """An fp32-state checkpoint loads into a bf16-state optimizer as the RNE rounding of the saved
    moments; a bf16-state checkpoint loads into an fp32-state optimizer exactly."""
    pa, oa = _make(gpu, BF16)
    assert oa.state_dtype == torch.float32
    _run(gpu, pa, oa, 0, 3)
    ck = _roundtrip(oa.state_dict())
    pb, ob = _make(gpu, BF16, state_dtype=BF16)
    ob.load_state_dict(ck)
    for k, p in enumerate(pb):
        st, e = ob.optimizer.state[p], ck["state"][k]
        assert e["exp_avg"].dtype == torch.float32 and st["exp_avg"].dtype == BF16
        for name in ("exp_avg", "exp_avg_sq"):
            _same(host(st[name]), zo.f32_to_bf16_bits(host(e[name]).view(np.float32)), f"{name} {k}")
        _same(host(st["master_residual"]), host(e["master_residual"]), f"residual {k}")
        assert int(st["step"].item()) == 3
    ck16 = _roundtrip(ob.state_dict())
    pc, oc = _make(gpu, BF16)
    oc.load_state_dict(ck16)
    for k, p in enumerate(pc):
        st = oc.optimizer.state[p]
        for name in ("exp_avg", "exp_avg_sq"):
            assert st[name].dtype == torch.float32
            _same(host(st[name]), zo.bf16_bits_to_f32(host(ck16["state"][k][name])), f"{name} {k}")


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_construction_and_step_errors(gpu, pg1):
    from zero_amd import zero1, zero2, zero3

    P = lambda: [torch.nn.Parameter(torch.zeros(8, device=gpu))]  # noqa: E731
    adam = lambda **kw: torch.optim.Adam(P(), **{**ADAM, **kw})  # noqa: E731
    for mod in (zero1, zero2):
        with pytest.raises(ValueError, match=r"beta2.*0\.99609375"):
            mod.ShardedOptimizer(torch.optim.Adam(P(), lr=1e-3), state_dtype=BF16)  # beta2 = 0.999
        with pytest.raises(ValueError, match=r"beta1.*0\.99609375"):
            mod.ShardedOptimizer(adam(betas=(0.999, 0.95)), state_dtype=BF16)
        with pytest.raises(ValueError, match="amsgrad"):
            mod.ShardedOptimizer(adam(amsgrad=True), state_dtype=BF16)
        with pytest.raises(ValueError, match="SGD"):
            mod.ShardedOptimizer(torch.optim.SGD(P(), lr=0.1, momentum=0.9), state_dtype=BF16)
        with pytest.raises(ValueError, match="bucket"):
            mod.ShardedOptimizer(adam(), state_dtype=BF16, arena="buckets")
        for bad in (torch.float16, torch.float64, "bf16"):
            with pytest.raises(ValueError, match="state_dtype"):
                mod.ShardedOptimizer(adam(), state_dtype=bad)
        assert mod.ShardedOptimizer(adam(), state_dtype=None).state_dtype == torch.float32
        assert mod.ShardedOptimizer(adam(), state_dtype=torch.float32).state_dtype == torch.float32
    with pytest.raises(ValueError, match="update"):
        zero3.ShardedOptimizer(adam(), update=False, state_dtype=BF16)
    with pytest.raises(ValueError, match=r"beta2.*0\.99609375"):
        zero3.ShardedOptimizer(torch.optim.Adam(P(), lr=1e-3), update=True, state_dtype=BF16)
    with pytest.raises(ValueError, match="amsgrad"):
        zero3.ShardedOptimizer(adam(amsgrad=True), update=True, state_dtype=BF16)
    with pytest.raises(ValueError, match="SGD"):
        zero3.ShardedOptimizer(torch.optim.SGD(P(), lr=0.1), update=True, state_dtype=BF16)
    with pytest.raises(ValueError, match="state_dtype"):
        zero3.ShardedOptimizer(adam(), update=True, state_dtype=torch.float16)
    # groups are mutable between steps: a beta moved past the bound, amsgrad switched on
    for mod in (zero1, zero2):
        opt = mod.ShardedOptimizer(adam(), state_dtype=BF16)
        p = opt.params[0]
        p.grad = torch.ones(8, device=gpu)
        opt.step()
        before = host(p), host(opt.optimizer.state[p]["exp_avg"])
        opt.original_param_groups[0]["betas"] = (0.9, 0.999)
        p.grad = torch.ones(8, device=gpu)
        with pytest.raises(ValueError, match=r"beta2.*0\.99609375"):
            opt.step()
        opt.original_param_groups[0]["betas"] = (0.9, 0.95)
        opt.original_param_groups[0]["amsgrad"] = True
        with pytest.raises(ValueError, match="amsgrad"):
            opt.step()
        torch.cuda.synchronize()
        assert np.array_equal(host(p), before[0])  # nothing ran
        assert np.array_equal(host(opt.optimizer.state[p]["exp_avg"]), before[1])
        assert int(opt.engine.steps[0]) == 1


def test_make_hp_carries_the_guard(gpu, pg1):
    from zero_amd._update import UpdateCore

    core = UpdateCore("adam", 64, gpu, 1, [0], 1, state_dtype=BF16)
    assert core.m.dtype == BF16 and core.v.dtype == BF16 and core.v.data_ptr() % 16 == 0
    hpd = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.0, amsgrad=False,
               maximize=False, decoupled=False)
    core.make_hp(hpd, 1)
    with pytest.raises(ValueError, match=r"beta2.*0\.99609375"):
        core.make_hp({**hpd, "beta2": 0.999}, 1)
    with pytest.raises(ValueError, match="amsgrad"):
        core.make_hp({**hpd, "amsgrad": True}, 1)
    with pytest.raises(ValueError, match="amsgrad"):
        core.ensure_vmax()
    with pytest.raises(ValueError, match="SGD"):
        UpdateCore("sgd", 64, gpu, 1, [0], 1, state_dtype=BF16)
    with pytest.raises(ValueError, match="carry"):
        UpdateCore("adam", 64, gpu, 2, [0], 1, carry=True, state_dtype=BF16)


# ---------------------------------------------------------------------------------------------
# world size 2 through real RCCL
# ---------------------------------------------------------------------------------------------
def _ws2_zero2_worker(rank, ws, port):
    """ZeRO-2 on the flat arena, bf16 split master: the reduced gradient is the bf16 rounding of
    the two-term fp32 sum; several rounds (4,096-element windows)."""
    from _gloo_comm import test_comm
    from zero_amd import zero2

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    shapes = [(100, 90), (64,), (4096 + 40,)]
    rng = np.random.default_rng(17)
    bits = lambda s, scale: zo.f32_to_bf16_bits((rng.standard_normal(s) * scale).astype(np.float32)).reshape(-1)  # noqa: E731
    init = [bits(s, 0.05) for s in shapes]
    dev_bf16 = lambda b, s: torch.from_numpy(b.view(np.int16).copy()).view(BF16).reshape(s).to(dev)  # noqa: E731
    params = [torch.nn.Parameter(dev_bf16(a, s)) for a, s in zip(init, shapes)]
    ref = [_Ref(a) for a in init]
    local = [[[bits(s, 1e-2) for s in shapes] for _ in range(ws)] for _ in range(3)]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, **ADAM), comm=test_comm(),
                                 bucket_mb=ws * 4096 * 2 / (1 << 20), state_dtype=BF16)
    assert opt.engine.split and opt.engine.K > 1 and opt.state_dtype == BF16
    for t in range(3):
        opt.zero_grad()
        for p, g, s in zip(params, local[t][rank], shapes):
            set_grad(p, dev_bf16(g, s))
        opt.step()
        for i, (p, r) in enumerate(zip(params, ref)):
            red = zo.f32_to_bf16_bits(zo.bf16_bits_to_f32(local[t][0][i]) + zo.bf16_bits_to_f32(local[t][1][i]))
            r.step(red, div=2.0)
            st = opt.optimizer.state[p] if i in opt.local_param_indices else None
            r.check(p, st, f"rank {rank} step {t} param {i}")
    dist.barrier()
    dist.destroy_process_group()


def _ws2_zero3_worker(rank, ws, port):
    """ZeRO-3 in update mode: one pass, two passes (the fp32 accumulation arena: the fp32-gradient
    split-master set with bf16 moments), one pass."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    opt = _zero3_schedule(rank, ws, torch.device("cuda:0"), test_comm(), (1, 2, 1),
                          grad_accumulation=True, accumulation_dtype=torch.float32)
    assert opt._acc_widen and {ck[3] for ck in opt._adam_cache} == {False, True}
    dist.barrier()
    dist.destroy_process_group()


def _ws2_zero1_refused_worker(rank, ws, port):
    """ZeRO-1 at world size 2 keeps the gradient carry: refused on every rank before anything
    collective (no communicator is passed; had the constructor gone on, it would have built one)."""
    from zero_amd import zero1

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    p = torch.nn.Parameter(torch.zeros(8, device="cuda:0"))
    with pytest.raises(ValueError, match="ZeRO-1"):
        zero1.ShardedOptimizer(torch.optim.Adam([p], **ADAM), state_dtype=BF16)
    dist.destroy_process_group()


def test_ws2_rccl(gpu, rccl_env):
    t0 = time.perf_counter()
    spawn_batch(2, [(_ws2_zero2_worker, ()), (_ws2_zero3_worker, ()),
                    (_ws2_zero1_refused_worker, ())], all_spawned=True)
    print(f"ws=2 bf16-state batch: {time.perf_counter() - t0:.1f} s")
