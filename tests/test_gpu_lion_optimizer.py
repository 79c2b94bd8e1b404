"""``ShardedOptimizer(zero_amd.optim.Lion(...))`` on ZeRO-1/2/3: the fused Lion behind the wrappers.

Every trajectory is compared bit for bit with tests/_lion_oracle.py stepping the same (reduced)
gradients; fp32 ones at world size 1 also with ``zero_amd.optim.Lion`` itself on the CPU.  Multi-rank
cases use small integer gradients that differ per rank, so the reduced sum is exact whatever the
order and the wire dtype.
"""
import copy

import numpy as np
import pytest
import torch
import torch.distributed as dist

import _lion_oracle as lo
from _zero_run import init_pg, module_for, set_grad, spawn_batch
from conftest import free_port

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SHAPES = [(1000, 7), (64,), (4097,), ()]
GROUPS = [([0, 1], dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.1)),
          ([2, 3], dict(lr=3e-4, betas=(0.95, 0.98)))]
SEED = 77


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


def _bits(a):
    a = np.ascontiguousarray(a).reshape(-1)
    return a.view(np.uint32 if a.itemsize == 4 else np.uint16)


def _host(t):
    """A device tensor as a flat numpy array (bf16 / int16: the uint16 bits)."""
    t = t.detach().cpu().contiguous().reshape(-1)
    if t.dtype in (torch.bfloat16, torch.int16):
        return t.view(torch.int16).numpy().view(np.uint16).copy()
    return t.numpy().copy()


def _to_dev(a, shape, kind, dev):
    """fp32 values (kind f32) or bf16 bits (kind split) as a device tensor of ``shape``."""
    if kind == "f32":
        return torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).reshape(shape).to(dev)
    return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).reshape(shape).to(dev)


def _init(rng, shapes, kind):
    out = []
    for s in shapes:
        a = (rng.standard_normal(s) * 0.1).astype(np.float32).reshape(-1)
        out.append(a if kind == "f32" else lo.f32_to_bf16_bits(a))
    return out


def _rand_grads(rng, shapes, kind):
    out = []
    for s in shapes:
        g = (rng.standard_normal(s) * 1e-2).astype(np.float32).reshape(-1)
        out.append(g if kind == "f32" else lo.f32_to_bf16_bits(g))
    return out


def _int_grads(rng, shapes, kind):
    """Integers in [-8, 8]: exact in bf16, and so is every sum of a few of them."""
    out = []
    for s in shapes:
        g = rng.integers(-8, 9, size=int(np.prod(s, dtype=np.int64))).astype(np.float32)
        out.append(g if kind == "f32" else lo.f32_to_bf16_bits(g))
    return out


def _sum(per_rank, kind):
    """The reduced gradient of one parameter: the exact sum over ranks, in the wire dtype."""
    vals = [g if kind == "f32" else lo.bf16_bits_to_f32(g) for g in per_rank]
    s = np.sum(np.stack(vals), axis=0, dtype=np.float32)
    return s if kind == "f32" else lo.f32_to_bf16_bits(s)


class _Ref:
    """The oracle over whole (flat) parameters: kind "f32" (fp32 params and grads), "split" (bf16
    params and grads, split master), "bf16" (bf16 params and grads, a separate fp32 master) or
    "bf16comm" (fp32 params whose gradients reach the update rounded to bf16).  ``state``: "f32",
    "bf16" or "sr" (``offs[i]``: parameter i's element 0 in the shard's momentum array)."""

    def __init__(self, init, groups, kind, ws=1, carry=False, state="f32", offs=None, seed=SEED):
        self.kind, self.ws, self.state, self.offs, self.seed = kind, ws, state, offs, seed
        self.cfg = {i: dict(kw) for idx, kw in groups for i in idx}
        if kind in ("f32", "bf16comm"):
            self.p = [a.copy() for a in init]
        elif kind == "bf16":
            self.p = [lo.bf16_bits_to_f32(a) for a in init]  # the fp32 master
            self.pb = [a.copy() for a in init]
        else:
            self.hi = [a.copy() for a in init]
            self.lo = [np.zeros(a.size, np.uint16) for a in init]  # master = the bf16 param exactly
        self.m = [np.zeros(a.size, np.float32 if state == "f32" else np.uint16) for a in init]
        self.steps = [0] * len(init)
        self.carry = [np.zeros(a.size, np.float32) for a in init] if carry else None

    def step(self, sums, coef=None, count_only=False):
        for i, g in enumerate(sums):
            if g is None:
                continue
            self.steps[i] += 1
            if count_only:  # a skipped step: the count (and with it the rounding key) alone
                continue
            c = self.cfg[i]
            hp = lo.LionHP(c["lr"], *c.get("betas", (0.9, 0.99)), c.get("weight_decay", 0.0),
                           maximize=c.get("maximize", False), grad_div=float(self.ws),
                           carry_mul=float(self.ws - 1) if self.carry is not None else 0.0)
            kw = dict(carry=None if self.carry is None else self.carry[i], coef=coef)
            if self.state == "sr":
                e = np.arange(self.offs[i], self.offs[i] + self.m[i].size, dtype=np.uint64)
                kw["sr"] = (e, lo.keys_of(self.seed, self.steps[i]))
            if self.kind == "f32":
                self.p[i], self.m[i], cr = lo.step_f32(self.p[i], g, self.m[i], hp, **kw)
            elif self.kind == "bf16comm":
                self.p[i], self.m[i], cr = lo.step_f32(self.p[i], lo.bf16_bits_to_f32(g), self.m[i],
                                                       hp, **kw)
            elif self.kind == "bf16":
                self.p[i], self.pb[i], self.m[i], cr = lo.step_bf16(self.p[i], g, self.m[i], hp, **kw)
            else:
                self.hi[i], self.lo[i], self.m[i], cr = lo.step_split(self.hi[i], self.lo[i], g,
                                                                      self.m[i], hp, **kw)
            if self.carry is not None:
                self.carry[i] = cr

    def param(self, i):
        return {"f32": lambda: self.p[i], "bf16comm": lambda: self.p[i], "bf16": lambda: self.pb[i],
                "split": lambda: self.hi[i]}[self.kind]()


def _same(got, want, what):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {_bits(want).size} differ, first at {bad[:8]}"


def _lion(params, groups):
    from zero_amd.optim import Lion

    return Lion([dict(params=[params[i] for i in idx], **g) for idx, g in groups])


def _make(variant, init, shapes, groups, kind, dev, **kw):
    params = [torch.nn.Parameter(_to_dev(a, s, kind, dev)) for a, s in zip(init, shapes)]
    return params, module_for(variant).ShardedOptimizer(_lion(params, groups), **kw)


def _offsets(opt, n):
    eng = opt.engine
    return [int(eng.pieces.stream_off[eng.pieces.param == i][0]) if (eng.pieces.param == i).any()
            else 0 for i in range(n)]


def _check_owned_state(opt, params, ref, what):
    """Parameters on every rank; exp_avg (and residuals, carry) where this rank owns them."""
    eng = opt.engine
    for i, p in enumerate(params):
        _same(_host(p), ref.param(i), f"{what} param {i}")
        if i not in opt.local_param_indices:
            continue
        st = opt.optimizer.state[p]
        assert {"exp_avg"} <= set(st) and "exp_avg_sq" not in st and st["exp_avg"].shape == p.shape
        assert st["exp_avg"].dtype == (torch.float32 if ref.state == "f32" else BF16)
        _same(_host(st["exp_avg"]), ref.m[i], f"{what} exp_avg {i}")
        if ref.steps[i]:
            assert float(st["step"]) == ref.steps[i]
        views = eng.state_views(i)
        if ref.kind == "split":
            _same(_host(views["master_residual"]), ref.lo[i], f"{what} residual {i}")
        if ref.kind == "bf16":
            _same(_host(views["master_param"]), ref.p[i], f"{what} master {i}")
        if ref.carry is not None:
            so_ = int(eng.pieces.stream_off[eng.pieces.param == i][0])
            _same(_host(eng.carry[so_:so_ + p.numel()]), ref.carry[i], f"{what} carry {i}")


def _run(opt, params, grads, shapes, kind, dev):
    opt.zero_grad()
    for p, g, s in zip(params, grads, shapes):
        p.grad = None if g is None else _to_dev(g, s, kind, dev)
    opt.step()


# ---------------------------------------------------------------------------------------------
# world size 1
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("kind", ["f32", "split"])
def test_ws1_two_groups_and_lr_schedule(gpu, pg1, variant, kind):
    """5 steps, two groups, a 0-d parameter, one parameter without a gradient in step 1, the first
    group's lr changed between steps (a scheduler mutates the group dicts)."""
    rng = np.random.default_rng(1)
    init = _init(rng, SHAPES, kind)
    params, opt = _make(variant, init, SHAPES, GROUPS, kind, gpu)
    groups = copy.deepcopy(GROUPS)
    ref = _Ref(init, groups, kind)
    eng = opt.engine
    assert eng.kind == "lion" and eng.v is None and eng.m.dtype == torch.float32
    assert eng.state.numel() == eng.L + (0 if kind == "f32" else (eng.L + 1) // 2)  # one moment
    cpu = None
    if kind == "f32":
        cpu = [torch.nn.Parameter(torch.from_numpy(a.copy()).reshape(s)) for a, s in zip(init, SHAPES)]
        cpu_opt = _lion(cpu, GROUPS)
    for t in range(5):
        grads = _rand_grads(rng, SHAPES, kind)
        if t == 0:
            grads[1] = None
        if t == 2:
            opt.param_groups[0]["lr"] = 5e-4
            for i in (0, 1):
                ref.cfg[i]["lr"] = 5e-4
            if cpu is not None:
                cpu_opt.param_groups[0]["lr"] = 5e-4
        _run(opt, params, grads, SHAPES, kind, gpu)
        ref.step(grads)
        _check_owned_state(opt, params, ref, f"step {t}")
        if cpu is not None:
            for q, g, s in zip(cpu, grads, SHAPES):
                q.grad = None if g is None else torch.from_numpy(g.copy()).reshape(s)
            cpu_opt.step()
            for i, (p, q) in enumerate(zip(params, cpu)):
                _same(_host(p), q.detach().numpy(), f"step {t} param {i} vs Lion on the CPU")
                if "exp_avg" in cpu_opt.state[q]:
                    _same(_host(opt.optimizer.state[p]["exp_avg"]),
                          cpu_opt.state[q]["exp_avg"].numpy(), f"step {t} exp_avg {i} vs Lion")
    assert ref.steps == [5, 4, 5, 5]


def test_ws1_fp32_master_and_bf16_exchange(gpu, pg1):
    """master="fp32" (bf16 parameters with a separate fp32 master and its bf16 copy) and
    grad_comm="bf16" (fp32 parameters whose gradients are rounded to bf16 for the exchange)."""
    for kind, kw in (("bf16", dict(master="fp32")), ("bf16comm", dict(grad_comm="bf16"))):
        rng = np.random.default_rng(6)
        store = "f32" if kind == "bf16comm" else "split"  # how parameters and gradients are held
        init = _init(rng, SHAPES, store)
        params, opt = _make(2, init, SHAPES, GROUPS, store, gpu, **kw)
        ref = _Ref(init, GROUPS, kind)
        assert not opt.engine.split and (opt.engine.master is not None) == (kind == "bf16")
        for t in range(3):
            grads = _rand_grads(rng, SHAPES, store)
            _run(opt, params, grads, SHAPES, store, gpu)
            ref.step([lo.f32_to_bf16_bits(g) for g in grads] if kind == "bf16comm" else grads)
            _check_owned_state(opt, params, ref, f"{kind} step {t}")


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
@pytest.mark.parametrize("kind", ["f32", "split"])
def test_ws1_bf16_state(gpu, pg1, kind, rounding):
    """bf16 exp_avg to nearest and stochastic; under one seed a second optimizer draws the same
    bits, under another seed other bits."""
    rng = np.random.default_rng(4)
    init = _init(rng, SHAPES, kind)
    steps = [_rand_grads(rng, SHAPES, kind) for _ in range(3)]
    kw = dict(state_dtype=BF16, state_rounding=rounding, state_seed=SEED)
    params, opt = _make(2, init, SHAPES, GROUPS, kind, gpu, **kw)
    eng = opt.engine
    assert eng.m.dtype == BF16 and eng.v is None
    words = (eng.L + 1) // 2
    assert eng.state.numel() == (words if kind == "f32" else (words + 3) // 4 * 4 + words)
    ref = _Ref(init, GROUPS, kind, state="sr" if rounding == "stochastic" else "bf16",
               offs=_offsets(opt, len(init)))
    for t, grads in enumerate(steps):
        _run(opt, params, grads, SHAPES, kind, gpu)
        ref.step(grads)
        _check_owned_state(opt, params, ref, f"{rounding} step {t}")
    if rounding == "stochastic":
        pb, ob = _make(2, init, SHAPES, GROUPS, kind, gpu, **kw)
        pc, oc = _make(2, init, SHAPES, GROUPS, kind, gpu, **dict(kw, state_seed=SEED + 1))
        for grads in steps:
            _run(ob, pb, grads, SHAPES, kind, gpu)
            _run(oc, pc, grads, SHAPES, kind, gpu)
        _same(_host(ob.engine.m), _host(eng.m), "the same seed")
        assert (_host(oc.engine.m) != _host(eng.m)).mean() > 0.2
        near = _Ref(init, GROUPS, kind, state="bf16")
        for grads in steps:
            near.step(grads)
        assert (ref.m[0] != near.m[0]).mean() > 0.2


@pytest.mark.parametrize("variant", [2, 3])
def test_ws1_clipping_skip_and_param_norms(gpu, pg1, variant):
    """max_grad_norm with param_grad_norms and skip_nonfinite: step 2 is clipped (coefficient about
    0.1), step 3 carries an inf gradient and is skipped -- parameters, residuals and exp_avg stay
    bit for bit, only the step count (and with it the rounding key) moves -- and step 4 goes on."""
    kind = "split"
    shapes = SHAPES if variant == 2 else Z3_SHAPES
    rng = np.random.default_rng(2)
    init = _init(rng, shapes, kind)
    steps = [_rand_grads(rng, shapes, kind) for _ in range(4)]
    f = lambda g: lo.bf16_bits_to_f32(g)  # noqa: E731
    steps[1] = [lo.f32_to_bf16_bits(f(g) * np.float32(40)) for g in steps[1]]
    steps[2][2] = steps[2][2].copy()
    steps[2][2][5] = 0x7F80  # +inf
    norm0 = float(np.sqrt(sum(np.sum(f(g).astype(np.float64) ** 2) for g in steps[0])))
    kw = dict(max_grad_norm=4.0 * norm0, skip_nonfinite=True, param_grad_norms=True,
              state_dtype=BF16, state_rounding="stochastic", state_seed=SEED)
    if variant == 3:
        kw["update"] = True
    params, opt = _make(variant, init, shapes, GROUPS, kind, gpu, **kw)
    offs = _offsets(opt, len(init)) if variant == 2 else [int(opt._arena.slot[i]) for i in range(4)]
    ref = _Ref(init, GROUPS, kind, state="sr", offs=offs)
    coefs = []
    for t, grads in enumerate(steps):
        before = [_host(p) for p in params]
        if variant == 2:
            _run(opt, params, grads, shapes, kind, gpu)
        else:
            for p, g, s in zip(params, grads, shapes):
                _z3_set_grad(p, _to_dev(g, s, kind, gpu))
            opt.step()
        coef = np.float32(opt.last_clip_coef.item())
        coefs.append(coef)
        ref.step(grads, coef=coef, count_only=bool(np.isnan(coef)))
        if variant == 2:
            _check_owned_state(opt, params, ref, f"step {t}")
        else:
            _z3_check(opt, params, ref, 1, 0, f"step {t}")
        if t == 2:
            for p, b in zip(params, before):
                _same(_host(p), b, "skipped step")
        else:
            want = [float(np.sqrt(np.sum(f(g).astype(np.float64) ** 2))) for g in grads]
            got = opt.last_param_grad_norms.cpu().numpy()
            assert np.allclose(got, want, rtol=1e-6, atol=0)
    assert coefs[0] == 1 and 0.05 < coefs[1] < 0.2 and np.isnan(coefs[2]) and coefs[3] == 1, coefs
    assert int(opt.skipped_steps.item()) == 1


def test_refused_configurations(gpu, pg1):
    from zero_amd import zero1, zero2, zero3
    from zero_amd.optim import Lion

    mk = lambda dt=torch.float32: [torch.nn.Parameter(torch.zeros(8, 4, device=gpu, dtype=dt))]  # noqa: E731
    for mod in (zero1, zero2, zero3):
        with pytest.raises(TypeError, match="Lion.*RMSprop"):
            mod.ShardedOptimizer(torch.optim.RMSprop(mk(), lr=1e-3))
    for mod in (zero1, zero2):
        with pytest.raises(ValueError, match="buckets"):
            mod.ShardedOptimizer(Lion(mk()), arena="buckets")
        with pytest.raises(ValueError, match="buckets"):
            mod.ShardedOptimizer(Lion(mk()), layout="chunk")
        with pytest.raises(ValueError, match="master='none'"):
            mod.ShardedOptimizer(Lion(mk(BF16)), master="none")
        with pytest.raises(ValueError, match="ema_decay"):
            mod.ShardedOptimizer(Lion(mk()), ema_decay=0.99)
        with pytest.raises(ValueError, match="param_update_norms"):
            mod.ShardedOptimizer(Lion(mk()), param_update_norms=True)
        with pytest.raises(ValueError, match=r"beta2 <= 0\.99609375"):
            mod.ShardedOptimizer(Lion(mk(), betas=(0.9, 0.999)), state_dtype=BF16)
        # beta1 is not bounded (it never reaches a stored value), and stochastic lifts beta2's bound
        mod.ShardedOptimizer(Lion(mk(), betas=(0.999, 0.99)), state_dtype=BF16)
        mod.ShardedOptimizer(Lion(mk(), betas=(0.9, 0.999)), state_dtype=BF16,
                             state_rounding="stochastic")
    with pytest.raises(ValueError, match="update mode"):
        zero3.ShardedOptimizer(Lion(mk()), update=False, state_dtype=BF16)
    for kw in (dict(master="none"), dict(ema_decay=0.9), dict(param_update_norms=True)):
        with pytest.raises(ValueError, match="Lion"):
            zero3.ShardedOptimizer(Lion(mk(BF16)), update=True, **kw)
    # a beta2 moved past the bound between steps is refused at the step, before anything runs
    opt = zero2.ShardedOptimizer(Lion(mk()), state_dtype=BF16)
    p = opt.params[0]
    p.grad = torch.ones(8, 4, device=gpu)
    opt.step()
    before = _host(p)
    assert torch.equal(p.detach().cpu(), torch.full((8, 4), float(-np.float32(1e-4))))
    opt.original_param_groups[0]["betas"] = (0.9, 0.999)
    p.grad = torch.ones(8, 4, device=gpu)
    with pytest.raises(ValueError, match=r"beta2 <= 0\.99609375"):
        opt.step()
    torch.cuda.synchronize()
    _same(_host(p), before, "refused step")


# ---------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,state", [("f32", "f32"), ("split", "sr")])
def test_checkpoint_zero2_ws1(gpu, pg1, kind, state):
    """3 steps + state_dict() + a fresh optimizer + load_state_dict() + 3 steps = 6 steps, bit for
    bit; the entries are exp_avg and step (and the residual)."""
    rng = np.random.default_rng(5)
    init = _init(rng, SHAPES, kind)
    steps = [_rand_grads(rng, SHAPES, kind) for _ in range(6)]
    kw = {} if state == "f32" else dict(state_dtype=BF16, state_rounding="stochastic",
                                        state_seed=SEED)
    pa, oa = _make(2, init, SHAPES, GROUPS, kind, gpu, **kw)
    for grads in steps:
        _run(oa, pa, grads, SHAPES, kind, gpu)
    pb, ob = _make(2, init, SHAPES, GROUPS, kind, gpu, **kw)
    for grads in steps[:3]:
        _run(ob, pb, grads, SHAPES, kind, gpu)
    sd = ob.state_dict()
    assert set(sd["state"]) == {0, 1, 2, 3}
    for e in sd["state"].values():
        assert {"exp_avg", "step"} <= set(e) and "exp_avg_sq" not in e and float(e["step"]) == 3
        assert ("master_residual" in e) == (kind == "split")
    now = [_host(p) for p in pb]
    pc, oc = _make(2, now, SHAPES, GROUPS, kind, gpu, **dict(kw, state_seed=0) if kw else {})
    oc.load_state_dict(sd)  # (the saved seed is adopted)
    for grads in steps[3:]:
        _run(oc, pc, grads, SHAPES, kind, gpu)
    for i, (a, c) in enumerate(zip(pa, pc)):
        _same(_host(c), _host(a), f"param {i}")
        _same(_host(oc.optimizer.state[c]["exp_avg"]), _host(oa.optimizer.state[a]["exp_avg"]),
              f"exp_avg {i}")
        assert float(oc.optimizer.state[c]["step"]) == 6


def test_checkpoint_from_unsharded_lion(gpu, pg1):
    """A plain ``Lion.state_dict()`` (fp32 CPU training) loads by index; the next step lands on the
    unsharded optimizer's bits."""
    rng = np.random.default_rng(9)
    init = _init(rng, SHAPES, "f32")
    steps = [_rand_grads(rng, SHAPES, "f32") for _ in range(4)]
    cpu = [torch.nn.Parameter(torch.from_numpy(a.copy()).reshape(s)) for a, s in zip(init, SHAPES)]
    cpu_opt = _lion(cpu, GROUPS)
    for grads in steps[:3]:
        for q, g, s in zip(cpu, grads, SHAPES):
            q.grad = torch.from_numpy(g.copy()).reshape(s)
        cpu_opt.step()
    sd = copy.deepcopy(cpu_opt.state_dict())
    params, opt = _make(2, [_host(q) for q in cpu], SHAPES, GROUPS, "f32", gpu)
    opt.load_state_dict(sd)
    assert [int(s) for s in opt.engine.steps] == [3, 3, 3, 3]
    _run(opt, params, steps[3], SHAPES, "f32", gpu)
    for q, g, s in zip(cpu, steps[3], SHAPES):
        q.grad = torch.from_numpy(g.copy()).reshape(s)
    cpu_opt.step()
    for i, (p, q) in enumerate(zip(params, cpu)):
        _same(_host(p), q.detach().numpy(), f"param {i}")
        _same(_host(opt.optimizer.state[p]["exp_avg"]), cpu_opt.state[q]["exp_avg"].numpy(), f"exp_avg {i}")
        assert float(opt.optimizer.state[p]["step"]) == 4


# ---------------------------------------------------------------------------------------------
# ZeRO-3 update mode
# ---------------------------------------------------------------------------------------------
Z3_SHAPES = [(5, 7), (64,), (130, 3), (1, 9)]


def _chunk_of(flat, shape, ws, rank):
    a = flat.reshape(shape)
    cs = -(-shape[0] // ws)
    return a[rank * cs:(rank + 1) * cs].reshape(-1)


def _z3_set_grad(p, g):
    """A full-size gradient on a sharded parameter, as autograd leaves it in the hook flow."""
    shard = p.data
    p.data = torch.empty(g.shape, dtype=g.dtype, device=g.device)
    p.grad = g
    p.data = shard


def _z3_check(opt, params, ref, ws, rank, what):
    for i, p in enumerate(params):
        _same(_host(p), _chunk_of(ref.param(i), Z3_SHAPES[i], ws, rank), f"{what} param {i}")
        st = opt.optimizer.state[p]
        if p.numel() == 0:
            continue
        assert "exp_avg" in st and "exp_avg_sq" not in st and st["exp_avg"].shape == p.shape
        _same(_host(st["exp_avg"]), _chunk_of(ref.m[i], Z3_SHAPES[i], ws, rank), f"{what} exp_avg {i}")
        if ref.steps[i]:
            assert float(st["step"]) == ref.steps[i]
        if ref.kind == "split":
            _same(_host(opt._state_views(i)["master_residual"]),
                  _chunk_of(ref.lo[i], Z3_SHAPES[i], ws, rank), f"{what} residual {i}")


def _z3_run(rank, ws, kind, state, dev, comm, ckpt):
    """ZeRO-3 update mode: 6 steps against the oracle on the summed gradients; ``ckpt``: a second
    optimizer saved after 3 steps, loaded into a third, which must land on the first's bits."""
    rng = np.random.default_rng(8)
    init = _init(rng, Z3_SHAPES, kind)
    local = [[_int_grads(rng, Z3_SHAPES, kind) for _ in range(ws)] for _ in range(6)]
    kw = dict(update=True) if comm is None else dict(update=True, comm=comm)
    if state == "bf16":
        kw["state_dtype"] = BF16

    def run(params, opt, ts, ref=None):
        for t in ts:
            for p, g, s in zip(params, local[t][rank], Z3_SHAPES):
                _z3_set_grad(p, _to_dev(g, s, kind, dev))
            opt.step()
            assert all(p.grad is None for p in params)
            if ref is not None:
                ref.step([_sum([local[t][r][i] for r in range(ws)], kind) for i in range(len(init))])
                _z3_check(opt, params, ref, ws, rank, f"rank {rank} step {t}")

    pa, oa = _make(3, init, Z3_SHAPES, GROUPS, kind, dev, **kw)
    assert oa._kind == "lion" and oa._core.v is None
    ref = _Ref(init, GROUPS, kind, ws=ws, state=state)
    run(pa, oa, range(6), ref)
    if not ckpt:
        return
    pb, ob = _make(3, init, Z3_SHAPES, GROUPS, kind, dev, **kw)
    run(pb, ob, range(3))
    sd = ob.state_dict()
    pc, oc = _make(3, init, Z3_SHAPES, GROUPS, kind, dev, **kw)
    with torch.no_grad():
        for c, b in zip(pc, pb):
            c.data.copy_(b.data)
    oc.load_state_dict(sd)
    run(pc, oc, range(3, 6))
    _z3_check(oc, pc, ref, ws, rank, f"rank {rank} after load")


@pytest.mark.parametrize("kind,state", [("f32", "f32"), ("split", "f32"), ("split", "bf16")])
def test_zero3_update_ws1(gpu, pg1, kind, state):
    _z3_run(0, 1, kind, state, gpu, None, ckpt=kind == "f32")


def _z3_worker(rank, ws, port, kind, state, ckpt):
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    _z3_run(rank, ws, kind, state, torch.device("cuda:0"), test_comm(), ckpt)
    dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------
# world sizes 2 and 3, ZeRO-1 and ZeRO-2
# ---------------------------------------------------------------------------------------------
MR_SHAPES = [(40, 9), (64,), (4097,), (), (130, 3)]
MR_GROUPS = [([0, 1, 2], dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.1)),
             ([3, 4], dict(lr=3e-4, betas=(0.95, 0.98)))]


def _mr_worker(rank, ws, port, variant, kind, state):
    """Integer gradients that differ per rank; ZeRO-1 keeps its carry through opt.zero_grad();
    64-element (fp32) / 128-element (bf16) windows, so several rounds."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20 + variant)
    init = _init(rng, MR_SHAPES, kind)
    kw = dict(state_dtype=BF16) if state == "bf16" else {}
    params, opt = _make(variant, init, MR_SHAPES, MR_GROUPS, kind, dev, comm=test_comm(),
                        bucket_mb=ws * 64 * 4 / (1 << 20), **kw)
    eng = opt.engine
    assert eng.kind == "lion" and eng.K > 1 and (eng.carry is not None) == (variant == 1)
    ref = _Ref(init, MR_GROUPS, kind, ws=ws, carry=variant == 1, state=state)
    for t in range(4):
        local = [_int_grads(rng, MR_SHAPES, kind) for _ in range(ws)]
        opt.zero_grad()
        for p, g, s in zip(params, local[rank], MR_SHAPES):
            set_grad(p, _to_dev(g, s, kind, dev))
        opt.step()
        ref.step([_sum([local[r][i] for r in range(ws)], kind) for i in range(len(init))])
        _check_owned_state(opt, params, ref, f"z{variant} ws{ws} rank {rank} step {t}")
    dist.destroy_process_group()


def _z1_bf16_refused_worker(rank, ws, port):
    """ZeRO-1 at world size > 1 keeps the gradient carry: bf16 momentum is refused on every rank
    before anything collective (no communicator is passed)."""
    from zero_amd import zero1
    from zero_amd.optim import Lion

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    p = torch.nn.Parameter(torch.zeros(8, device="cuda:0"))
    with pytest.raises(ValueError, match="ZeRO-1"):
        zero1.ShardedOptimizer(Lion([p]), state_dtype=BF16)
    dist.destroy_process_group()


def _z3_accumulate_worker(rank, ws, port, state):
    """ZeRO-3 ``grad_accumulation`` with ``accumulation_dtype=torch.float32`` over bf16 chunks: a
    step of one pass (the bf16 arena), one of two passes (the fp32 accumulation arena, read by the
    fp32-gradient instances over the split master) and one of one pass again, with the inputs and
    the accumulation oracle of tests/test_gpu_zero3_accumulate_fp32.py."""
    import _accum32_oracle as a32
    import test_gpu_zero3_accumulate_fp32 as z3t
    from _gloo_comm import test_comm
    from test_gpu_zero3_accumulate import Probe, ProbeModel, _rows
    from zero_amd import zero3

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    init = z3t._init_weights("bf16")
    model = ProbeModel([Probe(torch.from_numpy(w.copy()).to(dev, BF16)) for w in init])
    params = [m.weight for m in model.probes]
    groups = [(list(range(len(params))), dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.1))]
    kw = dict(state_dtype=BF16) if state == "bf16" else {}
    opt = zero3.ShardedOptimizer(_lion(params, groups), update=True, comm=test_comm(),
                                 bucket_mb=z3t.BUCKET_MB, grad_accumulation=True,
                                 accumulation_dtype=torch.float32, **kw)
    zero3.register_zero3_hooks(model, opt.param_managers)
    assert opt._acc_widen
    ref = _Ref([lo.f32_to_bf16_bits(w.reshape(-1)) for w in init], groups, "split", ws=ws, state=state)
    for step, npass in enumerate((1, 2, 1)):
        chunks = [[] for _ in params]
        for pas in range(npass):
            z3t._backward(model, step, pas, rank, dev)
            for i in range(len(params)):
                chunks[i].append(z3t.delivered(step, pas, i, ws))
        assert opt.accumulation_arena_dtype == (torch.float32 if npass >= 2 else BF16)
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        # (every module has a gradient in the first pass, so every parameter steps)
        ref.step([a32.accumulate_passes(c) if npass >= 2 else c[0] for c in chunks])
        for i, p in enumerate(params):
            what = f"rank {rank} step {step} param {i}"
            rows = lambda a, i=i: _rows(a, z3t.SHAPES[i], ws, rank)  # noqa: E731
            _same(_host(p), rows(ref.hi[i]), what)
            _same(_host(opt._state_views(i)["master_residual"]), rows(ref.lo[i]), what + " residual")
            _same(_host(opt.optimizer.state[p]["exp_avg"]), rows(ref.m[i]), what + " exp_avg")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_multirank_gloo(gpu, ws):
    if ws == 2:
        cases = [(_mr_worker, (2, "f32", "f32")), (_mr_worker, (2, "split", "bf16")),
                 (_z3_worker, ("f32", "f32", True)), (_z3_worker, ("split", "bf16", False)),
                 (_z3_accumulate_worker, ("f32",)), (_z3_accumulate_worker, ("bf16",)),
                 (_z1_bf16_refused_worker, ())]
    else:
        cases = [(_mr_worker, (1, "split", "f32")), (_mr_worker, (1, "f32", "f32"))]
    spawn_batch(ws, cases)


def test_ws2_real_rccl(gpu, rccl_env):
    """ZeRO-2 with bf16 parameters, the split master and bf16 momentum through the product
    communicator."""
    spawn_batch(2, [(_mr_worker, (2, "split", "bf16"))], all_spawned=True)
