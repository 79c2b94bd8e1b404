"""The fused Lion kernels (adam_segments_kernel / adam_scalar_kernel over LionRuleT) through
zero_amd.kernels.LionSet.

Every case runs 3 steps and compares every array the kernels may write, whole (gaps between
segments and 4,096 elements of slack behind the last one included), bit for bit against
tests/_lion_oracle.py.  C below is the chunk of the instance: 4,096 elements for the split master,
2,048 otherwise.  Kinds: "split" (bf16 gradient, split master), "bf16" (bf16 gradient, fp32 master
with its bf16 copy), "f32" (fp32 gradient, fp32 parameter in place), "f32split" (fp32 gradient over
the split master: ZeRO-3's fp32 accumulation arena).  State: "f32" momentum, "bf16" to nearest,
"sr" bf16 rounded stochastically.
"""
import numpy as np
import pytest
import torch

import _lion_oracle as lo
from oracle import c_oracle

pytestmark = pytest.mark.gpu

KINDS = ("split", "bf16", "f32", "f32split")
STATES = ("f32", "bf16", "sr")
CHUNK = {"split": 4096, "bf16": 2048, "f32": 2048, "f32split": 4096}
STEPS = 3
SLACK = 4096
SEED = 0x1234_5678_9ABC
# the tie classes of the split encoding, a denormal tie and neighbours of the bf16 overflow
# threshold, as tests/test_gpu_sgd_kernel.py plants them
TIES = np.array([0x3C808000, 0x3C818000, 0xBC808000, 0xBC818000, 0x00008000, 0x80008000,
                 0x7F7F7FFF, 0x7F7F8000, 0x3F80FFFF, 0x00000000], np.uint32)
HP = dict(lr=1e-3, beta1=0.9, beta2=0.99, weight_decay=0.1)


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


def _lengths(C):
    """The lengths {1, 3, 4, 5, 255, 257, C-1, C, C+1, 2C+7} plus an empty segment; the C+1 one is
    shifted by one element (the scalar table), the 257 one has no gradient."""
    return _layout([(1, True, 0), (3, True, 0), (4, True, 0), (0, True, 0), (5, True, 0),
                    (255, True, 0), (257, False, 0), (C - 1, True, 0), (C, True, 0),
                    (C + 1, True, 1), (2 * C + 7, True, 0)])


class _Case:
    def __init__(self, kind, state, segs, seed, hp=HP, *, carry=False, coef=None, guard=False,
                 repoint=False, N=None):
        self.kind, self.state, self.segs, self.hp = kind, state, segs, dict(hp)
        self.carry, self.coef, self.guard, self.repoint = carry, coef, guard, repoint
        self.split = kind in ("split", "f32split")
        self.g32 = kind in ("f32", "f32split")
        rng = np.random.default_rng(seed)
        self.N = N = (max(o + n for o, n, _ in segs) + SLACK) if N is None else N
        self.master0 = (rng.standard_normal(N) * 0.02).astype(np.float32)
        u = self.master0.view(np.uint32)
        for o, n, _ in segs:  # planted values at the head of every segment and of its second chunk
            for at in (o, o + CHUNK[kind]):
                k = max(0, min(len(TIES), o + n - at))
                u[at:at + k] = TIES[:k]
        m0 = (rng.standard_normal(N) * 5e-3).astype(np.float32)  # a momentum to interpolate with
        self.m0 = m0 if state == "f32" else lo.f32_to_bf16_bits(m0)
        self.grads = []
        for _ in range(STEPS):
            g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
            for o, n, _ in segs:  # c = +-0 over a zero momentum is planted by zeroing both
                if n >= 12:
                    g[o + 10], g[o + 11] = 0.0, -0.0
            self.grads.append(g if self.g32 else lo.f32_to_bf16_bits(g))
        for o, n, _ in segs:
            if n >= 12:
                self.m0[o + 10:o + 12] = 0

    def _hp(self, maker):
        return maker(**self.hp)

    def reference(self):
        N = self.N
        out = {"m": self.m0.copy()}
        if self.carry:
            out["carry"] = np.zeros(N, np.float32)
        if self.split:
            out["hi"], out["lo"] = c_oracle.split_master(self.master0)
        else:
            out["p"] = self.master0.copy()
            if self.kind == "bf16":
                out["pb"] = np.zeros(N, np.uint16)
        if self.coef is not None and np.isnan(self.coef):
            assert self.guard
            return out  # the guarded run with a NaN coefficient: nothing moves
        hp = self._hp(lo.LionHP)
        for t in range(1, STEPS + 1):
            keys = lo.keys_of(SEED, t)
            for o, n, has_g in self.segs:
                sl = slice(o, o + n)
                g = self.grads[t - 1][sl].copy()
                if not has_g:
                    g[:] = 0
                kw = dict(carry=out["carry"][sl] if self.carry else None, coef=self.coef)
                if self.state == "sr":  # the element's index in the momentum array
                    kw["sr"] = (np.arange(o, o + n, dtype=np.uint64), keys)
                if self.split:
                    out["hi"][sl], out["lo"][sl], out["m"][sl], cr = lo.step_split(
                        out["hi"][sl], out["lo"][sl], g, out["m"][sl], hp, **kw)
                elif self.kind == "bf16":
                    out["p"][sl], out["pb"][sl], out["m"][sl], cr = lo.step_bf16(
                        out["p"][sl], g, out["m"][sl], hp, **kw)
                else:
                    out["p"][sl], out["m"][sl], cr = lo.step_f32(out["p"][sl], g, out["m"][sl], hp, **kw)
                if self.carry:
                    out["carry"][sl] = cr
        return out

    def tensors(self, gpu):
        N = self.N
        dev = lambda a: torch.from_numpy(a.copy()).to(gpu)  # noqa: E731
        bits = lambda a: dev(a.view(np.int16))  # noqa: E731
        T = {"m": dev(self.m0) if self.state == "f32" else bits(self.m0)}
        if self.carry:
            T["carry"] = torch.zeros(N, device=gpu)
        if self.split:
            hi0, lo0 = c_oracle.split_master(self.master0)
            T["hi"], T["lo"] = bits(hi0), bits(lo0)
        else:
            T["p"] = dev(self.master0)
            if self.kind == "bf16":
                T["pb"] = torch.zeros(N, dtype=torch.int16, device=gpu)
        return T

    def rows(self, T, G):
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in self.segs:
            assert 0 <= o and o + n <= self.N - SLACK  # every segment inside the arrays
            g = G.data_ptr() + o * G.element_size() if has_g else 0
            if self.split:
                row = [g, at("hi", o), at("lo", o), at("hi", o)]
            else:
                row = [g, at("p", o), at("p", o), at("pb", o)]
            rows.append(row + [at("m", o), 0, 0, at("carry", o), n])
        return np.array(rows, dtype=np.uint64)

    def make_set(self, T, G):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import LionSet

        return LionSet(self.rows(T, G), ZS_F32 if self.g32 else ZS_BF16,
                       ZS_BF16_SPLIT if self.split else ZS_BF16, wide_grads=self.g32,
                       state_dtype=ZS_F32 if self.state == "f32" else ZS_BF16,
                       state_rounding="stochastic" if self.state == "sr" else "nearest")

    def run_gpu(self, gpu, loads_first=1, wg_per_cu=0):
        from zero_amd.kernels import lion_hparams, sr_keys

        T = self.tensors(gpu)
        gdt = torch.float32 if self.g32 else torch.int16
        Gs = [torch.zeros(self.N, dtype=gdt, device=gpu) for _ in range(STEPS if self.repoint else 1)]
        lset = self.make_set(T, Gs[0])
        coef = None if self.coef is None else torch.tensor([self.coef], dtype=torch.float32, device=gpu)
        st = torch.cuda.current_stream()
        _tune(b"adam_loads_first", loads_first)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            for t in range(1, STEPS + 1):
                g = self.grads[t - 1]
                G = Gs[(t - 1) % len(Gs)]
                G.copy_(torch.from_numpy(g if self.g32 else g.view(np.int16)))
                if self.repoint:  # the set walks from one gradient buffer to the next
                    lset.set_grads(self.rows(T, G)[:, 0], st)
                sr = (T["m"].data_ptr(), sr_keys(SEED, t)) if self.state == "sr" else None
                lset.run(self._hp(lion_hparams), st, coef=coef, guard=self.guard, sr=sr)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        return {k: v.cpu().numpy() for k, v in T.items()}


def _as_bits(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint16)


def _check(gpu, case, wg_per_cu=0, loads_first=(0, 1), want=None):
    want = case.reference() if want is None else want
    got = {}
    for lf in loads_first:
        got = case.run_gpu(gpu, lf, wg_per_cu)
        assert set(got) == set(want)
        for name, ref in want.items():
            bad = np.flatnonzero(_as_bits(got[name]) != _as_bits(ref))
            assert bad.size == 0, (f"{name}, adam_loads_first={lf}: {bad.size} elements differ from "
                                   f"the oracle, first at {bad[:8]}")
    return want, got


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kind", KINDS)
def test_lengths(gpu, kind, state):
    """Every length class in one set, with weight decay, adam_loads_first at 0 and 1; the segment
    without a gradient still decays its parameter and its momentum."""
    case = _Case(kind, state, _lengths(CHUNK[kind]), seed=3)
    want, _ = _check(gpu, case)
    o, n, has_g = case.segs[6]
    assert not has_g and n == 257
    if case.split:
        moved = c_oracle.join_master(want["hi"][o:o + n], want["lo"][o:o + n]) != case.master0[o:o + n]
    else:
        moved = want["p"][o:o + n] != case.master0[o:o + n]
    assert moved.mean() > 0.9
    assert (_as_bits(want["m"][o:o + n]) != _as_bits(case.m0[o:o + n])).mean() > 0.5


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kind", KINDS)
def test_clip_coefficient_and_guard(gpu, kind, state):
    """coef = 0.37 read from device memory multiplies the averaged gradient (grad_div 2); the
    guarded run with that coefficient gives the same bits, and with a NaN coefficient it leaves
    every byte as it was."""
    C = CHUNK[kind]
    segs = _layout([(2 * C + 6, True, 0), (300, True, 1), (5, False, 0)])
    hp = dict(HP, grad_div=2.0, maximize=True)
    c = float(np.float32(0.37))
    want, _ = _check(gpu, _Case(kind, state, segs, seed=19, hp=hp, coef=c), loads_first=(1,))
    _check(gpu, _Case(kind, state, segs, seed=19, hp=hp, coef=c, guard=True), want=want)
    skipped = _Case(kind, state, segs, seed=19, hp=hp, coef=float("nan"), guard=True)
    ref, got = _check(gpu, skipped)
    assert np.array_equal(_as_bits(got["m"]), _as_bits(skipped.m0))
    assert set(ref) == set(got)


@pytest.mark.parametrize("kind", ["split", "bf16", "f32"])
@pytest.mark.parametrize("div,mul", [(3.0, 2.0), (2.0, 1.0)])
def test_carry(gpu, kind, div, mul):
    """The ZeRO-1 carry (fp32 momentum only) with a true division (3) and a reciprocal multiply
    (2)."""
    C = CHUNK[kind]
    case = _Case(kind, "f32", _layout([(2 * C + 6, True, 0), (300, True, 1), (C + 4, False, 0)]),
                 seed=17, hp=dict(HP, grad_div=div, carry_mul=mul), carry=True)
    _check(gpu, case)


@pytest.mark.parametrize("kind", ["split", "f32", "f32split"])
def test_stochastic_rounding_does_not_depend_on_the_cut(gpu, kind):
    """The draw of an element is keyed by its index in the momentum array: the same array cut into
    other segments (one of them through the scalar table) gives the same bits."""
    C = CHUNK[kind]
    n = 3 * C + 40
    one = _Case(kind, "sr", [(0, n, True)], seed=31, N=n + SLACK)
    cut = _Case(kind, "sr", [(0, C + 8, True), (C + 8, 5, True), (C + 13, 2 * C + 27, True)],
                seed=31, N=n + SLACK)
    assert cut.segs[-1][0] % 4 == 1 and sum(s[1] for s in cut.segs) == n
    # (the planted values sit at the segment heads, which the cut moves: both cuts take one's)
    cut.master0, cut.m0, cut.grads = one.master0, one.m0, one.grads
    want, _ = _check(gpu, one, loads_first=(1,))
    assert all(np.array_equal(_as_bits(v), _as_bits(want[k])) for k, v in cut.reference().items())
    _check(gpu, cut, loads_first=(1,), want=want)
    nearest = _Case(kind, "bf16", [(0, n, True)], seed=31, N=n + SLACK).reference()
    assert (want["m"][:n] != nearest["m"][:n]).mean() > 0.2  # and it is not round-to-nearest


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("kind", ["split", "f32"])
def test_more_chunks_than_workgroups(gpu, kind, state):
    """300 chunks + 5 elements under one workgroup per CU: every workgroup walks several chunks."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert cus < 300
    n = 300 * CHUNK[kind] + 5
    _check(gpu, _Case(kind, state, [(0, n, True)], seed=5), wg_per_cu=1, loads_first=(1,))


@pytest.mark.parametrize("kind", ["split", "f32", "f32split"])
def test_set_grads_repoints_between_steps(gpu, kind):
    """Each step reads a gradient buffer of its own, bound with set_grads."""
    case = _Case(kind, "bf16", _lengths(CHUNK[kind]), seed=29, repoint=True)
    _check(gpu, case, loads_first=(1,))


@pytest.mark.parametrize("kind", KINDS)
def test_stats_count_the_lion_bytes(gpu, kind):
    """gradient + parameter read and write (+ bf16 copy) + momentum read and write."""
    n = CHUNK[kind] + 6
    gsz = 4 if kind in ("f32", "f32split") else 2
    param = {"split": 8, "f32split": 8, "bf16": 4 + 4 + 2, "f32": 4 + 4}[kind]
    for state, ssz in (("f32", 4), ("bf16", 2), ("sr", 2)):
        case = _Case(kind, state, [(0, n, True)], seed=1)
        T = case.tensors(gpu)
        G = torch.zeros(case.N, dtype=torch.float32 if case.g32 else torch.int16, device=gpu)
        lset = case.make_set(T, G)
        assert lset.elems == n and lset.bytes == n * (gsz + param + 2 * ssz)


def test_sqnorm_equals_the_adam_sets(gpu):
    """The sum-of-squares passes on a Lion set give the partials of an Adam set over the same
    gradients, bit for bit."""
    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT
    from zero_amd.kernels import AdamSet

    case = _Case("split", "f32", _lengths(4096), seed=23)
    T = case.tensors(gpu)
    G = torch.from_numpy(case.grads[0].view(np.int16)).to(gpu)
    rows = case.rows(T, G)
    lset = case.make_set(T, G)
    arows = rows.copy()
    V = torch.zeros(case.N, device=gpu)
    for r, (o, _, _) in zip(arows, case.segs):
        r[5] = V.data_ptr() + 4 * o
    aset = AdamSet(arows, ZS_BF16, ZS_BF16_SPLIT)
    assert lset.sqnorm_partials == aset.sqnorm_partials > 0 and lset.grad_bytes == aset.grad_bytes
    assert np.array_equal(lset.sqnorm_seg_offsets, aset.sqnorm_seg_offsets)
    st = torch.cuda.current_stream()
    pa = torch.full((aset.sqnorm_partials,), -1.0, dtype=torch.float64, device=gpu)
    pl = torch.full((lset.sqnorm_partials,), -2.0, dtype=torch.float64, device=gpu)
    sa = torch.full((int(aset.sqnorm_seg_offsets[-1]),), -1.0, dtype=torch.float64, device=gpu)
    sl = torch.full((int(lset.sqnorm_seg_offsets[-1]),), -2.0, dtype=torch.float64, device=gpu)
    aset.grad_sqnorm(pa, st)
    lset.grad_sqnorm(pl, st)
    aset.grad_sqnorm_segs(sa, st)
    lset.grad_sqnorm_segs(sl, st)
    torch.cuda.synchronize()
    assert np.array_equal(pa.cpu().numpy().view(np.uint64), pl.cpu().numpy().view(np.uint64))
    assert np.array_equal(sa.cpu().numpy().view(np.uint64), sl.cpu().numpy().view(np.uint64))


def test_invalid_calls_launch_nothing(gpu):
    """The ZS_ERR_INVALID cases that need a set with segments: each returns its code with a
    message and leaves the buffers as they were."""
    from zero_amd import _lib
    from zero_amd._lib import ZeroAmdError
    from zero_amd.kernels import LionSet, lion_hparams, sr_keys

    n = 2048 + 6
    mk = lambda: torch.randn(n + 64, device=gpu)  # noqa: E731
    p, g, m, carry = mk(), mk(), mk(), mk()
    m16 = torch.zeros(n + 64, dtype=torch.int16, device=gpu)
    coef = torch.tensor([0.5], device=gpu)
    row = lambda mm, **k: np.array([[g.data_ptr(), p.data_ptr(), p.data_ptr(), 0, mm, 0, 0,  # noqa: E731
                                     k.get("carry", 0), n]], np.uint64)
    F32, BF16 = _lib.ZS_F32, _lib.ZS_BF16
    with_carry = LionSet(row(m.data_ptr(), carry=carry.data_ptr()), F32, BF16)
    sr = LionSet(row(m16.data_ptr() + 64), F32, BF16, state_dtype=BF16, state_rounding="stochastic")
    plain = LionSet(row(m.data_ptr()), F32, BF16)
    st = torch.cuda.current_stream()
    torch.cuda.synchronize()
    before = [t.clone() for t in (p, g, m, carry, m16)]

    def refused(fn, *words):
        with pytest.raises(ZeroAmdError) as e:
            fn()
        assert e.value.code == _lib.ZS_ERR_INVALID
        assert all(w in str(e.value) for w in words), str(e.value)

    hp = lion_hparams(1e-3)
    keys = sr_keys(1, 1)
    refused(lambda: with_carry.run(hp, st, coef=coef), "carry")
    refused(lambda: sr.run(hp, st, sr=(m16.data_ptr() + 128, keys)), "below m_base")
    refused(lambda: sr.run(hp, st, sr=(m16.data_ptr() + 63, keys)), "odd byte distance")
    refused(lambda: sr.run(hp, st), "stochastic")
    refused(lambda: plain.run(hp, st, sr=(m.data_ptr(), keys)), "stochastic")
    refused(lambda: plain.run(hp, st, guard=True), "guard")
    refused(lambda: plain.run_sr(hp, 0, keys, st), "LionSet.run")
    refused(lambda: LionSet(row(m16.data_ptr(), carry=carry.data_ptr()), F32, BF16, state_dtype=BF16),
            "ZS_BF16 state", "carry")
    torch.cuda.synchronize()
    for t, b in zip((p, g, m, carry, m16), before):
        assert torch.equal(t.view(torch.int16), b.view(torch.int16))
