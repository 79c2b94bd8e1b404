"""``ShardedOptimizer(torch.optim.SGD(...))`` on ZeRO-1/2/3: the fused SGD behind the wrappers.

Every trajectory is compared bit for bit with tests/_sgd_oracle.py stepping the same (reduced)
gradients; fp32 ones at world size 1 also with ``torch.optim.SGD`` on the CPU.  Multi-rank cases use
small integer gradients that differ per rank, so the reduced sum is exact whatever the order and
the wire dtype.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _sgd_oracle as so
from _zero_run import init_pg, module_for, set_grad, spawn_batch
from conftest import free_port

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 7), (64,), (4097,), ()]
GROUPS = [([0, 1], dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
          ([2, 3], dict(lr=0.02, momentum=0.8, nesterov=True))]


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
        out.append(a if kind == "f32" else so.f32_to_bf16_bits(a))
    return out


def _rand_grads(rng, shapes, kind):
    out = []
    for s in shapes:
        g = (rng.standard_normal(s) * 1e-2).astype(np.float32).reshape(-1)
        out.append(g if kind == "f32" else so.f32_to_bf16_bits(g))
    return out


def _int_grads(rng, shapes, kind):
    """Integers in [-8, 8]: exact in bf16, and so is every sum of a few of them."""
    out = []
    for s in shapes:
        g = rng.integers(-8, 9, size=int(np.prod(s, dtype=np.int64))).astype(np.float32)
        out.append(g if kind == "f32" else so.f32_to_bf16_bits(g))
    return out


def _sum(per_rank, kind):
    """The reduced gradient of one parameter: the exact sum over ranks, in the wire dtype."""
    vals = [g if kind == "f32" else so.bf16_bits_to_f32(g) for g in per_rank]
    s = np.sum(np.stack(vals), axis=0, dtype=np.float32)
    return s if kind == "f32" else so.f32_to_bf16_bits(s)


class _Ref:
    """The oracle over whole (flat) parameters: kind "f32" (fp32 params and grads), "split" (bf16
    params and grads, split master), "bf16" (bf16 params and grads, a separate fp32 master) or
    "bf16comm" (fp32 params whose gradients reach the update rounded to bf16)."""

    def __init__(self, init, groups, kind, ws=1, carry=False):
        self.kind, self.ws = kind, ws
        self.cfg = {i: kw for idx, kw in groups for i in idx}
        n = len(init)
        if kind in ("f32", "bf16comm"):
            self.p = [a.copy() for a in init]
        elif kind == "bf16":
            self.p = [so.bf16_bits_to_f32(a) for a in init]  # the fp32 master
            self.pb = [a.copy() for a in init]
        else:
            self.hi = [a.copy() for a in init]
            self.lo = [np.zeros(a.size, np.uint16) for a in init]  # master = the bf16 param exactly
        self.buf = [None] * n
        self.steps = [0] * n
        self.carry = [np.zeros(a.size, np.float32) for a in init] if carry else None

    def step(self, sums, coef=None):
        for i, g in enumerate(sums):
            if g is None:
                continue
            self.steps[i] += 1
            hp = so.SgdHP(first=self.steps[i] == 1, grad_div=float(self.ws),
                          carry_mul=float(self.ws - 1) if self.carry is not None else 0.0,
                          **self.cfg[i])
            kw = dict(carry=None if self.carry is None else self.carry[i], coef=coef)
            if self.kind == "f32":
                self.p[i], self.buf[i], cr = so.step_f32(self.p[i], g, self.buf[i], hp, **kw)
            elif self.kind == "bf16comm":
                self.p[i], self.buf[i], cr = so.step_f32(self.p[i], so.bf16_bits_to_f32(g),
                                                         self.buf[i], hp, **kw)
            elif self.kind == "bf16":
                self.p[i], self.pb[i], self.buf[i], cr = so.step_bf16(self.p[i], g, self.buf[i], hp,
                                                                      **kw)
            else:
                self.hi[i], self.lo[i], self.buf[i], cr = so.step_split(self.hi[i], self.lo[i], g,
                                                                        self.buf[i], hp, **kw)
            if self.carry is not None:
                self.carry[i] = cr

    def param(self, i):
        return {"f32": lambda: self.p[i], "bf16comm": lambda: self.p[i], "bf16": lambda: self.pb[i],
                "split": lambda: self.hi[i]}[self.kind]()


def _same(got, want, what):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {_bits(want).size} differ, first at {bad[:8]}"


def _make(variant, init, shapes, groups, kind, dev, **kw):
    params = [torch.nn.Parameter(_to_dev(a, s, kind, dev)) for a, s in zip(init, shapes)]
    sgd = torch.optim.SGD([dict(params=[params[i] for i in idx], **g) for idx, g in groups], lr=1.0)
    return params, module_for(variant).ShardedOptimizer(sgd, **kw)


def _check_owned_state(opt, params, ref, what):
    """Parameters on every rank; buffers (and residuals) where this rank owns them."""
    eng = opt.engine
    for i, p in enumerate(params):
        _same(_host(p), ref.param(i), f"{what} param {i}")
        if i not in opt.local_param_indices:
            continue
        st = opt.optimizer.state[p]
        if ref.steps[i] == 0 or ref.buf[i] is None:
            assert "momentum_buffer" not in st
        else:
            assert set(st) == {"momentum_buffer"} and st["momentum_buffer"].shape == p.shape
            _same(_host(st["momentum_buffer"]), ref.buf[i], f"{what} buffer {i}")
        views = eng.state_views(i)
        if ref.kind == "split":
            _same(_host(views["master_residual"]), ref.lo[i], f"{what} residual {i}")
        if ref.kind == "bf16":
            _same(_host(views["master_param"]), ref.p[i], f"{what} master {i}")
        if ref.carry is not None:
            so_ = int(eng.pieces.stream_off[eng.pieces.param == i][0])
            _same(_host(eng.carry[so_:so_ + p.numel()]), ref.carry[i], f"{what} carry {i}")


# ---------------------------------------------------------------------------------------------
# world size 1
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "split"])
def test_ws1_zero2_two_groups(gpu, pg1, kind):
    """5 steps, two groups (momentum + weight decay; Nesterov with another lr), a 0-d parameter,
    one parameter without a gradient in step 1 (its first step is its group's second)."""
    rng = np.random.default_rng(1)
    init = _init(rng, SHAPES, kind)
    params, opt = _make(2, init, SHAPES, GROUPS, kind, gpu)
    ref = _Ref(init, GROUPS, kind)
    assert opt.engine.kind == "sgd" and opt.engine.v is None
    L = opt.engine.L  # one fp32 buffer (+ the int16 residuals): half of Adam's two moments
    assert opt.engine.state.numel() == L + (0 if kind == "f32" else (L + 1) // 2)
    assert all(len(opt.optimizer.state[p]) == 0 for p in params)  # empty before the first step
    cpu = None
    if kind == "f32":
        cpu = [torch.nn.Parameter(torch.from_numpy(a.copy()).reshape(s)) for a, s in zip(init, SHAPES)]
        cpu_opt = torch.optim.SGD([dict(params=[cpu[i] for i in idx], **g) for idx, g in GROUPS],
                                  lr=1.0, foreach=False)
    for t in range(5):
        grads = _rand_grads(rng, SHAPES, kind)
        if t == 0:
            grads[1] = None
        opt.zero_grad()
        for p, g, s in zip(params, grads, SHAPES):
            p.grad = None if g is None else _to_dev(g, s, kind, gpu)
        opt.step()
        ref.step(grads)
        _check_owned_state(opt, params, ref, f"step {t}")
        if cpu is not None:
            for q, g, s in zip(cpu, grads, SHAPES):
                q.grad = None if g is None else torch.from_numpy(g.copy()).reshape(s)
            cpu_opt.step()
            for i, (p, q) in enumerate(zip(params, cpu)):
                _same(_host(p), q.detach().numpy(), f"step {t} param {i} vs torch")
                tb = cpu_opt.state[q].get("momentum_buffer")
                if tb is not None:
                    _same(_host(opt.optimizer.state[p]["momentum_buffer"]), tb.numpy(),
                          f"step {t} buffer {i} vs torch")
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
            opt.zero_grad()
            for p, g, s in zip(params, grads, SHAPES):
                p.grad = _to_dev(g, s, store, gpu)
            opt.step()
            ref.step([so.f32_to_bf16_bits(g) for g in grads] if kind == "bf16comm" else grads)
            _check_owned_state(opt, params, ref, f"{kind} step {t}")


@pytest.mark.parametrize("variant", [1, 2])
def test_ws1_clipping_and_inf(gpu, pg1, variant):
    """max_grad_norm: a finite limit clips with the coefficient the device reports (about 0.1 in
    step 2), infinity leaves the bits of the unclipped run."""
    kind = "f32"
    rng = np.random.default_rng(2)
    init = _init(rng, SHAPES, kind)
    steps = [_rand_grads(rng, SHAPES, kind) for _ in range(3)]
    steps[1] = [(g * np.float32(40)).astype(np.float32) for g in steps[1]]
    norm0 = float(np.sqrt(sum(np.sum(g.astype(np.float64) ** 2) for g in steps[0])))
    out = {}
    for limit in (None, float("inf"), 4.0 * norm0):
        params, opt = _make(variant, init, SHAPES, GROUPS, kind, gpu, max_grad_norm=limit)
        ref = _Ref(init, GROUPS, kind)
        coefs = []
        for t, grads in enumerate(steps):
            opt.zero_grad()
            for p, g, s in zip(params, grads, SHAPES):
                p.grad = _to_dev(g, s, kind, gpu)
            opt.step()
            coef = None
            if limit is not None:
                want = float(np.sqrt(sum(np.sum(g.astype(np.float64) ** 2) for g in grads)))
                assert abs(float(opt.last_grad_norm.item()) - want) <= 1e-6 * want
                coef = np.float32(opt.last_clip_coef.item())
                coefs.append(coef)
            ref.step(grads, coef=coef)
            _check_owned_state(opt, params, ref, f"limit {limit} step {t}")
        if limit is not None and np.isfinite(limit):
            assert coefs[0] == 1 and coefs[2] == 1 and 0.05 < coefs[1] < 0.2, coefs
        elif limit is not None:
            assert all(c == 1 for c in coefs)
        out[limit] = [_host(p) for p in params] + [_host(opt.optimizer.state[p]["momentum_buffer"])
                                                   for p in params]
    for a, b in zip(out[None], out[float("inf")]):
        _same(a, b, "inf vs None")


@pytest.mark.parametrize("kind", ["f32", "split"])
def test_momentum_zero_allocates_no_state(gpu, pg1, kind):
    rng = np.random.default_rng(3)
    groups = [([0, 1], dict(lr=0.1, weight_decay=1e-2)), ([2, 3], dict(lr=0.05, maximize=True))]
    init = _init(rng, SHAPES, kind)
    params, opt = _make(2, init, SHAPES, groups, kind, gpu)
    ref = _Ref(init, groups, kind)
    eng = opt.engine
    assert eng.m is None and eng.v is None
    # nothing but the split master's int16 residuals (none for fp32 parameters)
    assert eng.state.numel() == (0 if kind == "f32" else (eng.L + 1) // 2)
    for t in range(3):
        grads = _rand_grads(rng, SHAPES, kind)
        opt.zero_grad()
        for p, g, s in zip(params, grads, SHAPES):
            p.grad = _to_dev(g, s, kind, gpu)
        opt.step()
        ref.step(grads)
        _check_owned_state(opt, params, ref, f"step {t}")
    assert all(len(opt.optimizer.state[p]) == 0 for p in params)
    # a momentum that appears after construction has no buffer to live in
    opt.param_groups[0]["momentum"] = 0.9
    for p, g, s in zip(params, grads, SHAPES):
        p.grad = _to_dev(g, s, kind, gpu)
    before = [_host(p) for p in params]
    with pytest.raises(ValueError, match="momentum"):
        opt.step()
    torch.cuda.synchronize()
    for p, b in zip(params[:2], before[:2]):
        _same(_host(p), b, "refused step")


def test_refused_configurations(gpu, pg1):
    from zero_amd import zero1, zero2, zero3

    mk = lambda: [torch.nn.Parameter(torch.zeros(8, 4, device=gpu))]  # noqa: E731
    for mod in (zero1, zero2, zero3):
        with pytest.raises(TypeError, match="RMSprop"):
            mod.ShardedOptimizer(torch.optim.RMSprop(mk(), lr=1e-3))
    with pytest.raises(ValueError, match="buckets"):
        zero2.ShardedOptimizer(torch.optim.SGD(mk(), lr=0.1), arena="buckets")
    with pytest.raises(ValueError, match="buckets"):
        zero2.ShardedOptimizer(torch.optim.SGD(mk(), lr=0.1), layout="chunk")
    with pytest.raises(ValueError, match="differentiable"):
        zero2.ShardedOptimizer(torch.optim.SGD(mk(), lr=0.1, differentiable=True))
    opt = zero2.ShardedOptimizer(torch.optim.SGD(mk(), lr=torch.tensor(0.1)))  # a tensor lr: .item()
    opt.params[0].grad = torch.ones(8, 4, device=gpu)
    opt.step()
    want = torch.full((8, 4), float(-np.float32(0.1)), dtype=torch.float32)
    assert torch.equal(opt.params[0].detach().cpu(), want)


# ---------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "split"])
def test_checkpoint_zero2_ws1(gpu, pg1, kind):
    """3 steps + state_dict() + a fresh optimizer + load_state_dict() + 3 steps = 6 steps, bit for
    bit; the dict is torch's SGD format; a state without buffers makes every parameter first again."""
    rng = np.random.default_rng(5)
    init = _init(rng, SHAPES, kind)
    steps = [_rand_grads(rng, SHAPES, kind) for _ in range(6)]

    def run(params, opt, which):
        for grads in which:
            opt.zero_grad()
            for p, g, s in zip(params, grads, SHAPES):
                p.grad = _to_dev(g, s, kind, gpu)
            opt.step()

    pa, oa = _make(2, init, SHAPES, GROUPS, kind, gpu)
    run(pa, oa, steps)
    pb, ob = _make(2, init, SHAPES, GROUPS, kind, gpu)
    run(pb, ob, steps[:3])
    sd = ob.state_dict()
    assert set(sd["state"]) == {0, 1, 2, 3}
    for e in sd["state"].values():
        assert "momentum_buffer" in e and "step" not in e and e["momentum_buffer"].dtype == torch.float32
        assert ("master_residual" in e) == (kind == "split")
    now = [_host(p) for p in pb]
    pc, oc = _make(2, now, SHAPES, GROUPS, kind, gpu)
    oc.load_state_dict(sd)
    assert all("momentum_buffer" in oc.optimizer.state[p] for p in pc)
    run(pc, oc, steps[3:])
    for i, (a, c) in enumerate(zip(pa, pc)):
        _same(_host(c), _host(a), f"param {i}")
        _same(_host(oc.optimizer.state[c]["momentum_buffer"]),
              _host(oa.optimizer.state[a]["momentum_buffer"]), f"buffer {i}")
        if kind == "split":
            _same(_host(oc.engine.state_views(i)["master_residual"]),
                  _host(oa.engine.state_views(i)["master_residual"]), f"residual {i}")
    # without buffers: first again (the stale buffer contents are not read)
    for e in sd["state"].values():
        del e["momentum_buffer"]
    pd, od = _make(2, now, SHAPES, GROUPS, kind, gpu)
    od.engine.m.fill_(3.0)
    od.load_state_dict(sd)
    assert all(len(od.optimizer.state[p]) == 0 for p in pd) and not od.engine.steps.any()
    ref = _Ref(now, GROUPS, kind)
    if kind == "split":
        ref.lo = [_host(sd["state"][i]["master_residual"]) for i in range(4)]
    run(pd, od, steps[3:4])
    ref.step(steps[3])
    _check_owned_state(od, pd, ref, "first again")


# ---------------------------------------------------------------------------------------------
# ZeRO-3 update mode
# ---------------------------------------------------------------------------------------------
Z3_SHAPES = [(5, 7), (64,), (130, 3), (1, 9)]
Z3_GROUPS = [([0, 1], dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
             ([2, 3], dict(lr=0.02, momentum=0.8, nesterov=True))]


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
        if ref.steps[i] == 0:
            assert "momentum_buffer" not in st
            continue
        assert set(st) == {"momentum_buffer"} and st["momentum_buffer"].shape == p.shape
        _same(_host(st["momentum_buffer"]), _chunk_of(ref.buf[i], Z3_SHAPES[i], ws, rank),
              f"{what} buffer {i}")
        if ref.kind == "split":
            _same(_host(opt._state_views(i)["master_residual"]),
                  _chunk_of(ref.lo[i], Z3_SHAPES[i], ws, rank), f"{what} residual {i}")


def _z3_run(rank, ws, kind, dev, comm, ckpt):
    """ZeRO-3 update mode: 6 steps against the oracle on the summed gradients; ``ckpt``: a second
    optimizer saved after 3 steps, loaded into a third, which must land on the first's bits."""
    rng = np.random.default_rng(8)
    init = _init(rng, Z3_SHAPES, kind)
    local = [[_int_grads(rng, Z3_SHAPES, kind) for _ in range(ws)] for _ in range(6)]
    kw = dict(update=True) if comm is None else dict(update=True, comm=comm)

    def run(params, opt, ts, ref=None):
        for t in ts:
            for p, g, s in zip(params, local[t][rank], Z3_SHAPES):
                _z3_set_grad(p, _to_dev(g, s, kind, dev))
            opt.step()
            assert all(p.grad is None for p in params)
            if ref is not None:
                ref.step([_sum([local[t][r][i] for r in range(ws)], kind) for i in range(len(init))])
                _z3_check(opt, params, ref, ws, rank, f"rank {rank} step {t}")

    pa, oa = _make(3, init, Z3_SHAPES, Z3_GROUPS, kind, dev, **kw)
    assert oa._kind == "sgd" and oa._v is None
    assert all(len(oa.optimizer.state[p]) == 0 for p in pa)
    assert tuple(pa[0].shape) == ((3, 7) if rank == 0 else (2, 7)) if ws == 2 else True
    ref = _Ref(init, Z3_GROUPS, kind, ws=ws)
    run(pa, oa, range(6), ref)
    if not ckpt:
        return
    pb, ob = _make(3, init, Z3_SHAPES, Z3_GROUPS, kind, dev, **kw)
    run(pb, ob, range(3))
    sd = ob.state_dict()
    for k, e in sd["state"].items():  # (rank 1's chunk of the one-row parameter is empty)
        assert "step" not in e and ("momentum_buffer" in e) == (pb[k].numel() > 0)
    pc, oc = _make(3, init, Z3_SHAPES, Z3_GROUPS, kind, dev, **kw)
    with torch.no_grad():
        for c, b in zip(pc, pb):
            c.data.copy_(b.data)
    oc.load_state_dict(sd)
    run(pc, oc, range(3, 6))
    _z3_check(oc, pc, ref, ws, rank, f"rank {rank} after load")


@pytest.mark.parametrize("kind", ["f32", "split"])
def test_zero3_update_ws1(gpu, pg1, kind):
    _z3_run(0, 1, kind, gpu, None, ckpt=False)


def _z3_worker(rank, ws, port, kind, ckpt):
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    _z3_run(rank, ws, kind, torch.device("cuda:0"), test_comm(), ckpt)
    dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------
# world sizes 2 and 3, ZeRO-1 and ZeRO-2
# ---------------------------------------------------------------------------------------------
MR_SHAPES = [(40, 9), (64,), (4097,), (), (130, 3)]
MR_GROUPS = [([0, 1, 2], dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
             ([3, 4], dict(lr=0.02, momentum=0.8, nesterov=True))]


def _mr_worker(rank, ws, port, variant, kind):
    """Integer gradients that differ per rank; ZeRO-1 keeps its carry through opt.zero_grad();
    64-element (fp32) / 128-element (bf16) windows, so several rounds."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(20 + variant)
    init = _init(rng, MR_SHAPES, kind)
    params, opt = _make(variant, init, MR_SHAPES, MR_GROUPS, kind, dev, comm=test_comm(),
                        bucket_mb=ws * 64 * 4 / (1 << 20))
    eng = opt.engine
    assert eng.kind == "sgd" and eng.K > 1 and (eng.carry is not None) == (variant == 1)
    ref = _Ref(init, MR_GROUPS, kind, ws=ws, carry=variant == 1)
    for t in range(4):
        local = [_int_grads(rng, MR_SHAPES, kind) for _ in range(ws)]
        opt.zero_grad()
        for p, g, s in zip(params, local[rank], MR_SHAPES):
            set_grad(p, _to_dev(g, s, kind, dev))
        opt.step()
        ref.step([_sum([local[r][i] for r in range(ws)], kind) for i in range(len(init))])
        _check_owned_state(opt, params, ref, f"z{variant} ws{ws} rank {rank} step {t}")
    dist.destroy_process_group()


def _backward_worker(rank, ws, port, kw, kind):
    """ZeRO-2 with the gradients from a real backward (loss = sum <p, G>, so p.grad == G exactly):
    ``overlap=True`` reduces them from the post-accumulate hooks, ``layout="flat"`` is the balanced
    Layout F (a parameter may straddle two owners, so only the parameters are compared)."""
    from _gloo_comm import test_comm

    torch.cuda.set_device(0)
    init_pg(rank, ws, port)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    init = _init(rng, MR_SHAPES, kind)
    params, opt = _make(2, init, MR_SHAPES, MR_GROUPS, kind, dev, comm=test_comm(),
                        bucket_mb=ws * 64 * 4 / (1 << 20), **kw)
    assert opt.engine.kind == "sgd" and opt.engine.arena_kind == "flat"
    ref = _Ref(init, MR_GROUPS, kind, ws=ws)
    for t in range(4):
        local = [_int_grads(rng, MR_SHAPES, kind) for _ in range(ws)]
        opt.zero_grad()
        gs = [_to_dev(g, s, kind, dev) for g, s in zip(local[rank], MR_SHAPES)]
        sum((p.float() * g.float()).sum() for p, g in zip(params, gs)).backward()
        opt.step()
        ref.step([_sum([local[r][i] for r in range(ws)], kind) for i in range(len(init))])
        if "layout" in kw:
            for i, p in enumerate(params):
                _same(_host(p), ref.param(i), f"layout F rank {rank} step {t} param {i}")
        else:
            _check_owned_state(opt, params, ref, f"overlap rank {rank} step {t}")
    dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_multirank_gloo(gpu, ws):
    kinds = ("f32", "split") if ws == 2 else ("split", "f32")  # (ZeRO-2's, ZeRO-1's)
    cases = [(_mr_worker, (2, kinds[0])), (_mr_worker, (1, kinds[1]))]
    if ws == 2:
        cases += [(_z3_worker, ("f32", True)), (_z3_worker, ("split", False))]
    else:
        cases += [(_backward_worker, (dict(overlap=True), "split")),
                  (_backward_worker, (dict(layout="flat"), "f32"))]
    spawn_batch(ws, cases)


def test_ws2_real_rccl(gpu, rccl_env):
    """ZeRO-2 with bf16 parameters and the split master through the product communicator."""
    spawn_batch(2, [(_mr_worker, (2, "split"))], all_spawned=True)
