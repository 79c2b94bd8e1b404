"""The fused SGD kernels (adam_segments_kernel / adam_scalar_kernel over SgdRule) through
zero_amd.kernels.SgdSet.

Every case runs 3 steps (the first with ``first`` set, so both branches of the momentum buffer
run) and compares every array the kernels may write, whole (gaps between segments and the slack
behind the last one included), bit for bit against tests/_sgd_oracle.py.  C below is the chunk of
the instance: 4,096 elements for the split master, 2,048 otherwise.
"""
import ctypes

import numpy as np
import pytest
import torch

import _sgd_oracle as so
from oracle import c_oracle

pytestmark = pytest.mark.gpu

KINDS = ("split", "bf16", "f32")  # bf16 grad + split master / bf16 grad + fp32 master / fp32 grad
CHUNK = {"split": 4096, "bf16": 2048, "f32": 2048}
STEPS = 3
SLACK = 4096
# the tie classes of the split encoding, a denormal tie and neighbours of the bf16 overflow
# threshold, as tests/test_gpu_adam_chunks.py plants them
TIES = np.array([0x3C808000, 0x3C818000, 0xBC808000, 0xBC818000, 0x00008000, 0x80008000,
                 0x7F7F7FFF, 0x7F7F8000, 0x3F80FFFF, 0x00000000], np.uint32)
MOM = dict(lr=0.05, momentum=0.9)


def _tune(key, value):
    from zero_amd import _lib

    _lib.call("zs_tune", key, int(value), None)


def _layout(spec):
    """[(n, has_grad, shift)] -> [(offset, n, has_grad)]: 16-byte aligned starts, `shift` elements
    off for a segment that must take the scalar table."""
    segs, off = [], 0
    for n, has_g, shift in spec:
        off = (off + 3) // 4 * 4 + shift
        segs.append((off, n, has_g))
        off += n
    return segs


class _Case:
    def __init__(self, kind, segs, seed, hp, *, buffers=None, carry=False, coef=None, repoint=False):
        self.kind, self.segs, self.hp, self.carry, self.coef = kind, segs, dict(hp), carry, coef
        self.buffers = bool(hp.get("momentum")) if buffers is None else buffers
        self.repoint = repoint
        rng = np.random.default_rng(seed)
        self.N = N = max(o + n for o, n, _ in segs) + SLACK
        self.master0 = (rng.standard_normal(N) * 0.02).astype(np.float32)
        u = self.master0.view(np.uint32)
        for o, n, _ in segs:  # planted values at the head of every segment and of its second chunk
            for at in (o, o + CHUNK[kind]):
                k = max(0, min(len(TIES), o + n - at))
                u[at:at + k] = TIES[:k]
        self.buf0 = (rng.standard_normal(N) * 7).astype(np.float32)  # stale: `first` must not read it
        self.grads = []
        for _ in range(STEPS):
            g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
            self.grads.append(g if kind == "f32" else so.f32_to_bf16_bits(g))

    def _hp(self, t, maker):
        return maker(first=t == 1, **self.hp)

    def reference(self):
        N, kind = self.N, self.kind
        out = {}
        if self.buffers:
            out["buf"] = self.buf0.copy()
        if self.carry:
            out["carry"] = np.zeros(N, np.float32)
        if kind == "split":
            out["hi"], out["lo"] = c_oracle.split_master(self.master0)
        else:
            out["p"] = self.master0.copy()
            if kind == "bf16":
                out["pb"] = np.zeros(N, np.uint16)
        use_buf = self.buffers and self.hp.get("momentum", 0.0) != 0
        for t in range(1, STEPS + 1):
            hp = self._hp(t, so.SgdHP)
            for o, n, has_g in self.segs:
                sl = slice(o, o + n)
                g = self.grads[t - 1][sl].copy()
                if not has_g:
                    g[:] = 0
                kw = dict(carry=out["carry"][sl] if self.carry else None, coef=self.coef)
                buf = out["buf"][sl] if use_buf else None
                if kind == "split":
                    out["hi"][sl], out["lo"][sl], buf, cr = so.step_split(out["hi"][sl], out["lo"][sl],
                                                                         g, buf, hp, **kw)
                elif kind == "bf16":
                    out["p"][sl], out["pb"][sl], buf, cr = so.step_bf16(out["p"][sl], g, buf, hp, **kw)
                else:
                    out["p"][sl], buf, cr = so.step_f32(out["p"][sl], g, buf, hp, **kw)
                if use_buf:
                    out["buf"][sl] = buf
                if self.carry:
                    out["carry"][sl] = cr
        return out

    def tensors(self, gpu):
        N, kind = self.N, self.kind
        dev = lambda a: torch.from_numpy(a.copy()).to(gpu)  # noqa: E731
        bits = lambda a: dev(a.view(np.int16))  # noqa: E731
        T = {}
        if self.buffers:
            T["buf"] = dev(self.buf0)
        if self.carry:
            T["carry"] = torch.zeros(N, device=gpu)
        if kind == "split":
            hi0, lo0 = c_oracle.split_master(self.master0)
            T["hi"], T["lo"] = bits(hi0), bits(lo0)
        else:
            T["p"] = dev(self.master0)
            if kind == "bf16":
                T["pb"] = torch.zeros(N, dtype=torch.int16, device=gpu)
        return T

    def rows(self, T, G):
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in self.segs:
            assert 0 <= o and o + n <= self.N - SLACK  # every segment inside the arrays
            g = G.data_ptr() + o * G.element_size() if has_g else 0
            if self.kind == "split":
                row = [g, at("hi", o), at("lo", o), at("hi", o)]
            else:
                row = [g, at("p", o), at("p", o), at("pb", o)]
            rows.append(row + [at("buf", o), 0, 0, at("carry", o), n])
        return np.array(rows, dtype=np.uint64)

    def dtypes(self):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32

        return (ZS_F32 if self.kind == "f32" else ZS_BF16,
                ZS_BF16_SPLIT if self.kind == "split" else ZS_BF16)

    def run_gpu(self, gpu, loads_first=1, wg_per_cu=0):
        from zero_amd.kernels import SgdSet, sgd_hparams

        T = self.tensors(gpu)
        gdt = torch.float32 if self.kind == "f32" else torch.int16
        Gs = [torch.zeros(self.N, dtype=gdt, device=gpu) for _ in range(STEPS if self.repoint else 1)]
        sset = SgdSet(self.rows(T, Gs[0]), *self.dtypes())
        coef = None if self.coef is None else torch.tensor([self.coef], dtype=torch.float32, device=gpu)
        st = torch.cuda.current_stream()
        _tune(b"adam_loads_first", loads_first)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            for t in range(1, STEPS + 1):
                g = self.grads[t - 1]
                G = Gs[(t - 1) % len(Gs)]
                G.copy_(torch.from_numpy(g if self.kind == "f32" else g.view(np.int16)))
                if self.repoint:  # the set walks from one gradient buffer to the next
                    sset.set_grads(self.rows(T, G)[:, 0], st)
                sset.run(self._hp(t, sgd_hparams), st, coef=coef)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        return {k: v.cpu().numpy() for k, v in T.items()}


def _as_bits(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint16)


def _check(gpu, case, wg_per_cu=0, loads_first=(0, 1)):
    want = case.reference()
    got = {}
    for lf in loads_first:
        got = case.run_gpu(gpu, lf, wg_per_cu)
        assert set(got) == set(want)
        for name, ref in want.items():
            bad = np.flatnonzero(_as_bits(got[name]) != _as_bits(ref))
            assert bad.size == 0, (f"{name}, adam_loads_first={lf}: {bad.size} elements differ from "
                                   f"the oracle, first at {bad[:8]}")
    return want, got


def _mixed(C):
    return _layout([(C + 400 + 3, True, 0),   # a full chunk, a partial chunk, a 3-element tail
                    (3, True, 0),             # shorter than one vector access
                    (C + 7, True, 1),         # misaligned gradient and arrays: the scalar table
                    (C + 4 + 1, False, 0),    # no gradient: momentum and weight decay still move it
                    (2 * C + 2, True, 0)])


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_set(gpu, kind):
    """Full and partial chunks, tails of 1-3 elements, a 3-element segment, a misaligned segment
    and a segment without a gradient in one set, with momentum and weight decay; the planted
    split-master ties, denormals and overflow neighbours sit at the head of every segment."""
    C = CHUNK[kind]
    case = _Case(kind, _mixed(C), seed=3, hp=dict(MOM, weight_decay=1e-2))
    want, _ = _check(gpu, case)
    o, n, has_g = case.segs[3]
    assert not has_g
    if kind == "split":
        moved = c_oracle.join_master(want["hi"][o:o + n], want["lo"][o:o + n]) != case.master0[o:o + n]
    else:
        moved = want["p"][o:o + n] != case.master0[o:o + n]
    assert moved.mean() > 0.9  # p - lr * (wd * p + momentum terms), all but the planted zero


@pytest.mark.parametrize("kind", ["split", "f32"])
@pytest.mark.parametrize("loads_first", [1, 0])
def test_more_chunks_than_workgroups(gpu, kind, loads_first):
    """One workgroup per CU over 2 * CUs + 3 chunks: every workgroup strides at least twice."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    C = CHUNK[kind]
    n = (2 * cus + 2) * C + 40  # 2 * cus + 2 full chunks and a partial one
    assert -(-n // C) == 2 * cus + 3
    _check(gpu, _Case(kind, [(0, n, True)], seed=5, hp=MOM), wg_per_cu=1, loads_first=(loads_first,))


HPS = {
    "mom0": dict(lr=0.1),
    "mom0.9": dict(lr=0.05, momentum=0.9),
    "damp0.1": dict(lr=0.05, momentum=0.9, dampening=0.1),
    "nesterov": dict(lr=0.02, momentum=0.8, nesterov=True),
    "wd": dict(lr=0.1, momentum=0.9, weight_decay=1e-2),
    "wd_mom0": dict(lr=0.1, weight_decay=1e-2),
    "maximize": dict(lr=0.05, momentum=0.9, maximize=True),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(HPS))
def test_hyperparameters(gpu, kind, name):
    """One hyper-parameter at a time at 2C + 4 + 2 (full chunks, a partial one, a tail).  A set
    without buffers (momentum 0) has no state array at all."""
    C = CHUNK[kind]
    case = _Case(kind, [(0, 2 * C + 6, True)], seed=11, hp=HPS[name])
    assert case.buffers == ("momentum" in HPS[name])
    _check(gpu, case)


@pytest.mark.parametrize("kind", ["split", "f32"])
def test_momentum_zero_leaves_buffers_alone(gpu, kind):
    """A set that has buffers, run with momentum 0 (a momentum-0 group in an arena that has a
    buffer): torch makes no buffer then, and the stale contents stay bit for bit."""
    C = CHUNK[kind]
    case = _Case(kind, [(0, C + 6, True)], seed=12, hp=dict(lr=0.1, dampening=0.5), buffers=True)
    want, got = _check(gpu, case)
    assert np.array_equal(_as_bits(got["buf"]), _as_bits(case.buf0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("div,mul", [(3.0, 2.0), (2.0, 1.0)])
def test_carry(gpu, kind, div, mul):
    """The ZeRO-1 carry with a true division (3) and a reciprocal multiply (2)."""
    C = CHUNK[kind]
    case = _Case(kind, _layout([(2 * C + 6, True, 0), (300, True, 1)]), seed=17,
                 hp=dict(MOM, grad_div=div, carry_mul=mul), carry=True)
    _check(gpu, case)


@pytest.mark.parametrize("kind", KINDS)
def test_carry_without_momentum(gpu, kind):
    C = CHUNK[kind]
    case = _Case(kind, [(0, C + 6, True)], seed=18, hp=dict(lr=0.1, grad_div=3.0, carry_mul=2.0),
                 carry=True)
    _check(gpu, case)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mom", [0.9, 0.0])
def test_clip_coefficient_from_device(gpu, kind, mom):
    """coef = 0.37 read from device memory multiplies the averaged gradient (grad_div 2)."""
    C = CHUNK[kind]
    hp = dict(lr=0.05, momentum=mom, weight_decay=1e-3, grad_div=2.0)
    case = _Case(kind, _layout([(2 * C + 6, True, 0), (300, True, 1)]), seed=19, hp=hp,
                 coef=float(np.float32(0.37)))
    _check(gpu, case)


@pytest.mark.parametrize("kind", KINDS)
def test_sqnorm_equals_the_adam_sets(gpu, kind):
    """The sum-of-squares pass on an SGD set gives the partials of an Adam set over the same
    gradients, bit for bit."""
    from zero_amd.kernels import AdamSet, SgdSet

    case = _Case(kind, _mixed(CHUNK[kind]), seed=23, hp=MOM)
    T = case.tensors(gpu)
    g = case.grads[0]
    G = torch.from_numpy(g if kind == "f32" else g.view(np.int16)).to(gpu)
    rows = case.rows(T, G)
    sset = SgdSet(rows, *case.dtypes())
    arows = rows.copy()
    V = torch.zeros(case.N, device=gpu)
    for r, (o, _, _) in zip(arows, case.segs):
        r[5] = V.data_ptr() + 4 * o
    aset = AdamSet(arows, *case.dtypes())
    assert sset.sqnorm_partials == aset.sqnorm_partials > 0
    assert sset.grad_bytes == aset.grad_bytes
    st = torch.cuda.current_stream()
    pa = torch.full((aset.sqnorm_partials,), -1.0, dtype=torch.float64, device=gpu)
    ps = torch.full((sset.sqnorm_partials,), -2.0, dtype=torch.float64, device=gpu)
    aset.grad_sqnorm(pa, st)
    sset.grad_sqnorm(ps, st)
    torch.cuda.synchronize()
    assert np.array_equal(pa.cpu().numpy().view(np.uint64), ps.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("kind", ["split", "f32"])
def test_set_grads_repoints_between_steps(gpu, kind):
    """Each step reads a gradient buffer of its own, bound with set_grads."""
    case = _Case(kind, _mixed(CHUNK[kind]), seed=29, hp=MOM, repoint=True)
    _check(gpu, case, loads_first=(1,))


@pytest.mark.parametrize("kind", KINDS)
def test_stats_count_the_sgd_bytes(gpu, kind):
    """gradient + parameter read and write (+ bf16 copy) + buffer read and write if present."""
    n = CHUNK[kind] + 6
    gsz = 4 if kind == "f32" else 2
    param = {"split": 2 + 2 + 2 + 2, "bf16": 4 + 4 + 2, "f32": 4 + 4}[kind]
    for hp, state in ((MOM, 8), (dict(lr=0.1), 0)):
        from zero_amd.kernels import SgdSet

        case = _Case(kind, [(0, n, True)], seed=1, hp=hp)
        T = case.tensors(gpu)
        G = torch.zeros(case.N, dtype=torch.float32 if kind == "f32" else torch.int16, device=gpu)
        sset = SgdSet(case.rows(T, G), *case.dtypes())
        assert sset.elems == n and sset.bytes == n * (gsz + param + state)


def test_invalid_calls_launch_nothing(gpu):
    """Every ZS_ERR_INVALID case returns its code with a message and leaves the buffers as they
    were."""
    from zero_amd import _lib
    from zero_amd._lib import SgdHParams, ZeroAmdError
    from zero_amd.kernels import AdamSet, SgdSet, adam_hparams, sgd_hparams

    n = 2048 + 6
    mk = lambda: torch.randn(n + 64, device=gpu)  # noqa: E731
    p, g, m, v, carry = mk(), mk(), mk(), mk(), mk()
    coef = torch.tensor([0.5], device=gpu)
    row = lambda **k: np.array([[g.data_ptr(), p.data_ptr(), p.data_ptr(), 0, k.get("m", 0),  # noqa: E731
                                 k.get("v", 0), k.get("vmax", 0), k.get("carry", 0), n]], np.uint64)
    F32, BF16 = _lib.ZS_F32, _lib.ZS_BF16
    with_buf = SgdSet(row(m=m.data_ptr()), F32, BF16)
    no_buf = SgdSet(row(), F32, BF16)
    with_carry = SgdSet(row(m=m.data_ptr(), carry=carry.data_ptr()), F32, BF16)
    adam = AdamSet(row(m=m.data_ptr(), v=v.data_ptr()), F32, BF16)
    st = torch.cuda.current_stream()
    torch.cuda.synchronize()
    before = [t.clone() for t in (p, g, m, v, carry)]

    def refused(fn, *words):
        with pytest.raises(ZeroAmdError) as e:
            fn()
        assert e.value.code == _lib.ZS_ERR_INVALID
        text = str(e.value)
        assert all(w in text for w in words), text

    ok = sgd_hparams(0.1, 0.9)
    ahp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    refused(lambda: _lib.call("zs_adamset_run", with_buf._h, ctypes.byref(ahp), int(st.cuda_stream)),
            "zs_adamset_run", "zs_sgdset_create")
    refused(lambda: _lib.call("zs_adamset_run_clipped", with_buf._h, ctypes.byref(ahp),
                              coef.data_ptr(), int(st.cuda_stream)), "zs_adamset_run_clipped")
    refused(lambda: _lib.call("zs_sgdset_run", adam._h, ctypes.byref(ok), None, int(st.cuda_stream)),
            "zs_sgdset_run", "zs_adamset_create")
    refused(lambda: no_buf.run(ok, st), "momentum", "without")
    refused(lambda: with_carry.run(ok, st, coef=coef), "carry")
    # torch's constructor rules, at the initialiser ...
    refused(lambda: sgd_hparams(0.1, 0.0, nesterov=True), "Nesterov")
    refused(lambda: sgd_hparams(0.1, 0.9, 0.1, nesterov=True), "Nesterov")
    refused(lambda: sgd_hparams(-0.1), "learning rate")
    refused(lambda: sgd_hparams(0.1, -0.5), "momentum")
    refused(lambda: sgd_hparams(0.1, 0.0, 0.0, -1e-2), "weight_decay")
    # ... and at the run, for a struct filled by hand
    def hand(**k):
        hp = SgdHParams(neg_lr=-0.1, momentum=0.9, one_minus_dampening=1.0, weight_decay=0.0,
                        grad_div=1.0, carry_mul=0.0, nesterov=0, maximize=0, first=0)
        for name, val in k.items():
            setattr(hp, name, val)
        return hp

    def unchanged():
        torch.cuda.synchronize()
        for t, b in zip((p, g, m, v, carry), before):
            assert torch.equal(t.view(torch.int32), b.view(torch.int32))

    unchanged()
    with_buf.run(hand(), st)  # the struct itself is fine
    torch.cuda.synchronize()
    assert not torch.equal(p, before[0])
    before = [t.clone() for t in (p, g, m, v, carry)]
    refused(lambda: with_buf.run(hand(neg_lr=0.1), st), "learning rate")
    refused(lambda: with_buf.run(hand(momentum=-0.9), st), "momentum")
    refused(lambda: with_buf.run(hand(weight_decay=-1.0), st), "weight_decay")
    refused(lambda: with_buf.run(hand(nesterov=1, momentum=0.0), st), "Nesterov")
    refused(lambda: with_buf.run(hand(nesterov=1, one_minus_dampening=0.9), st), "Nesterov")
    # zs_sgdset_create: v / vmax must be 0, m on all segments or none
    refused(lambda: SgdSet(row(m=m.data_ptr(), v=v.data_ptr()), F32, BF16), "zs_sgdset_create")
    two = np.concatenate([row(m=m.data_ptr()), row()])
    refused(lambda: SgdSet(two, F32, BF16), "all segments or none")
    unchanged()
