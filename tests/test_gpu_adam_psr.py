"""The master-free fused Adam kernels (p_dtype ZS_BF16_SR, zs_adamset_run_psr), bit for bit on every
element of p / m / v against the restatement of tests/_psr_oracle.py.

The model is tests/test_gpu_adam_bf16_state.py: segments (offset, n, has_grad) in one flat arena
that all arrays share, every array the kernel writes compared whole (gaps between segments and the
slack behind the last one included), with ``adam_loads_first`` at 0 and at 1, against the oracle and
against each other.  A NaN need only be a NaN.  The instances: gradient {bf16, fp32} x moments {fp32,
bf16 to nearest, bf16 stochastic}; the chunk C is the split master's, whose geometry they share.
``m_base`` = the address of the m arena less ``shift`` elements of its type, so the element at arena
offset o has index ``shift + o``.
"""
import numpy as np
import pytest
import torch

import _adam_space as sp
import _psr_oracle as po
import test_gpu_adam_bf16_state as nb
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_adam_chunks import SLACK, _mixed_table, _tune

pytestmark = pytest.mark.gpu

C = nb.CHUNK["split"]
GDT = ("bf16", "fp32")
STATES = po.STATES
BYTES = {("bf16", "bf16"): 14, ("bf16", "f32"): 22, ("fp32", "bf16"): 16, ("fp32", "f32"): 24}
SEED = (0xC0FFEE << 32) | 0x1234567
CLIP_COEF = nb.CLIP_COEF
combos = pytest.mark.parametrize("gdt,state", [(g, s) for g in GDT for s in STATES])


def _hp(**kw):
    return {**sp.DEFAULT, **kw}


class _Case:
    def __init__(self, gdt, state, segs, grads, hps, *, p0, m0=None, v0=None, shift=0, seed=SEED,
                 clip=False, div=1.0):
        self.gdt, self.state, self.segs, self.grads, self.hps = gdt, state, segs, grads, hps
        self.shift, self.seed, self.clip, self.div = int(shift), int(seed), clip, float(div)
        self.N = N = max(o + n for o, n, _ in segs) + SLACK
        assert all(len(g) == N for g in grads) and len(p0) == N
        z = np.zeros(N, np.float32)
        m0, v0 = z if m0 is None else m0, z if v0 is None else v0
        narrow = (lambda a: np.ascontiguousarray(a, np.float32).copy()) if state == "f32" \
            else zo.f32_to_bf16_bits
        self.state0 = {"p": zo.f32_to_bf16_bits(p0), "m": narrow(m0), "v": narrow(v0)}

    @classmethod
    def random(cls, gdt, state, segs, seed, steps=3, hp=None, **kw):
        rng = np.random.default_rng(seed)
        N = max(o + n for o, n, _ in segs) + SLACK
        p0 = (rng.standard_normal(N) * 0.02).astype(np.float32)
        grads = []
        for _ in range(steps):
            g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
            grads.append(g if gdt == "fp32" else zo.f32_to_bf16_bits(g))
        hps = [_hp(step=t, **(hp or {})) for t in range(1, steps + 1)]
        return cls(gdt, state, segs, grads, hps, p0=p0, **kw)

    @staticmethod
    def canon(out):
        return {k: sp.canon(np.ascontiguousarray(a)) for k, a in out.items()}

    def reference(self, coefs=None):
        out = {k: a.copy() for k, a in self.state0.items()}
        for t, (hp, G) in enumerate(zip(self.hps, self.grads)):
            chp = c_oracle.hparams(grad_div=1.0 if self.clip else self.div, **hp)
            keys = po.keys_of(self.seed, hp["step"])
            for o, n, has_g in self.segs:
                sl = slice(o, o + n)
                e = np.arange(n, dtype=np.uint64) + np.uint64(self.shift + o)
                g = G[sl].copy()
                if not has_g:
                    g[:] = 0
                if self.clip:
                    gf = g if self.gdt == "fp32" else zo.bf16_bits_to_f32(g)
                    with np.errstate(all="ignore"):
                        g = np.ascontiguousarray((gf / np.float32(self.div)).astype(np.float32)
                                                 * np.float32(coefs[t]))
                po.step(out["p"][sl], g, out["m"][sl], out["v"][sl], chp, e, keys, self.state)
        return self.canon(out)

    def build(self, gpu, bind=True):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SR, ZS_F32
        from zero_amd.kernels import AdamSet

        T = {k: torch.from_numpy(a.view(np.int16) if a.itemsize == 2 else a.copy()).to(gpu)
             for k, a in self.state0.items()}
        G = torch.zeros(self.N, dtype=torch.float32 if self.gdt == "fp32" else torch.int16,
                        device=gpu)
        at = lambda t, o: t.data_ptr() + o * t.element_size()  # noqa: E731
        rows = [[at(G, o) if has_g and bind else 0, at(T["p"], o), 0, at(T["p"], o), at(T["m"], o),
                 at(T["v"], o), 0, 0, n] for o, n, has_g in self.segs]
        aset = AdamSet(np.array(rows, dtype=np.uint64), ZS_F32 if self.gdt == "fp32" else ZS_BF16,
                       ZS_BF16_SR, wide_grads=self.gdt == "fp32",
                       state_dtype=ZS_F32 if self.state == "f32" else ZS_BF16,
                       state_rounding="stochastic" if self.state == "bf16_sr" else "nearest")
        return T, G, aset

    def m_base(self, T):
        base = T["m"].data_ptr() - T["m"].element_size() * self.shift
        assert base > 0
        return base

    def upload(self, G, g):
        G.copy_(torch.from_numpy(g if self.gdt == "fp32" else g.view(np.int16)))

    @staticmethod
    def ahp(h, div):
        from zero_amd.kernels import adam_hparams

        return adam_hparams(h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["step"],
                            decoupled=h["decoupled"], maximize=h["maximize"], grad_div=div)

    def download(self, T):
        out = {k: v.cpu().numpy() for k, v in T.items()}
        return self.canon({k: a.view(np.uint16) if a.itemsize == 2 else a for k, a in out.items()})

    def run_gpu(self, gpu, loads_first, wg_per_cu=0, max_norm=None, guard=False):
        from zero_amd.kernels import clip_coef, sqnorm_reduce, sr_keys

        T, G, aset = self.build(gpu)
        m_base = self.m_base(T)
        st = torch.cuda.current_stream()
        partials = torch.zeros(aset.sqnorm_partials + 8, dtype=torch.float64, device=gpu)
        sumsq, out2 = torch.zeros(1, device=gpu), torch.zeros(2, device=gpu)
        coefs = []
        _tune(b"adam_loads_first", loads_first)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            for h, g in zip(self.hps, self.grads):
                self.upload(G, g)
                hp, keys = self.ahp(h, self.div), sr_keys(self.seed, h["step"])
                if self.clip == "fixed":
                    out2.copy_(torch.from_numpy(np.array([0.0, CLIP_COEF], np.float32)))
                    aset.run_psr(hp, m_base, keys, st, coef=out2.data_ptr() + 4, guard=guard)
                    coefs.append(CLIP_COEF)
                elif self.clip:
                    aset.grad_sqnorm(partials, st)
                    sqnorm_reduce(partials, aset.sqnorm_partials, sumsq, st)
                    clip_coef(sumsq, self.div, max_norm, out2, st)
                    aset.run_psr(hp, m_base, keys, st, coef=out2.data_ptr() + 4, guard=guard)
                    torch.cuda.synchronize()
                    coefs.append(np.float32(out2.cpu().numpy()[1]))
                else:
                    aset.run_psr(hp, m_base, keys, st)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        return self.download(T), coefs

    def max_norm(self):
        """Half the L2 norm of the first step's averaged gradient: every step is clipped."""
        g = self.grads[0]
        x = (g if self.gdt == "fp32" else zo.bf16_bits_to_f32(g)).astype(np.float64)
        ss = sum(float(np.sum(x[o:o + n] ** 2)) for o, n, has_g in self.segs if has_g)
        return 0.5 * np.sqrt(ss) / self.div


def _check(gpu, case, wg_per_cu=0, guard=False):
    max_norm = case.max_norm() if case.clip is True else None
    got = {lf: case.run_gpu(gpu, lf, wg_per_cu, max_norm, guard) for lf in (0, 1)}
    coefs = got[1][1]
    if case.clip:
        print("coefficients", [float(c) for c in coefs])
        assert [c.tobytes() for c in got[0][1]] == [c.tobytes() for c in coefs]
        assert all(0.0 < c < 1.0 for c in coefs)
    want = case.reference(coefs)
    for name, ref in want.items():
        for lf in (0, 1):
            bad = np.flatnonzero(got[lf][0][name] != ref)
            assert bad.size == 0, (f"{name}, adam_loads_first={lf}: {bad.size} elements differ from "
                                   f"the oracle, first at {bad[:8]}")
        assert np.array_equal(got[0][0][name], got[1][0][name]), name
    return want


def _four_segments():
    """3C+5: three full chunks, a predicated partial one and a scalar tail; exactly one chunk;
    4 * 256 - 1: one partial group short of a lane access and a 3-element tail; C+1 one element (2
    bytes of the parameter) off alignment: scalar throughout."""
    segs, off = [], 0
    for n, shift in ((3 * C + 5, 0), (C, 0), (4 * 256 - 1, 0), (C + 1, 1)):
        off = (off + 3) // 4 * 4 + shift
        segs.append((off, n, True))
        off += n
    return segs


@combos
def test_four_segments(gpu, gdt, state):
    """Every instance over three steps keyed 1 to 3, AdamW on: full chunks, the predicated body,
    the scalar kernel on tails and on the misaligned segment."""
    case = _Case.random(gdt, state, _four_segments(), seed=71,
                        hp=dict(weight_decay=1e-2, decoupled=True))
    want = _check(gpu, case)
    assert (want["p"][:3 * C] != case.state0["p"][:3 * C]).mean() > 0.5  # (it did step)


@combos
def test_single_segments(gpu, gdt, state):
    """One segment of n = 1, 3, C - 1: scalar only; scalar only; predicated groups and a tail."""
    for k, n in enumerate((1, 3, C - 1)):
        _check(gpu, _Case.random(gdt, state, [(0, n, True)], seed=80 + k, steps=2))


@combos
def test_index_crosses_2_to_the_32(gpu, gdt, state):
    """m_base (2^32 - 5000) elements below the arena: the index passes 2^32 inside the first
    segment's second full chunk and every later element carries a high word of 1 — in the
    parameter's draw and, for stochastic moments, in theirs."""
    segs = _four_segments()
    assert C < 5000 < 2 * C < segs[0][1]
    case = _Case.random(gdt, state, segs, seed=72, shift=(1 << 32) - 5000)
    low = _Case.random(gdt, state, segs, seed=72, shift=0)
    want, other = _check(gpu, case), low.reference()
    n = segs[0][1]
    assert (want["p"][:n] != other["p"][:n]).mean() > 0.1  # other draws
    if state == "bf16_sr":
        assert (want["m"][:n] != other["m"][:n]).mean() > 0.1
    else:
        assert np.array_equal(want["m"], other["m"])


@pytest.mark.parametrize("gdt,state", [("bf16", "bf16_sr"), ("fp32", "f32"), ("bf16", "bf16")])
def test_several_chunks_per_workgroup(gpu, gdt, state):
    """tests/test_gpu_adam_chunks.py's mixed table (a segment without a gradient and a misaligned
    one in it) with one workgroup per CU: the grid is smaller than the chunk count, so every
    workgroup walks several chunks and segments, and the indices do not depend on the grid."""
    segs = _mixed_table(C)
    chunks = sum(n // C for _, n, _ in segs)
    assert 2 * torch.cuda.get_device_properties(gpu).multi_processor_count <= chunks
    _check(gpu, _Case.random(gdt, state, segs, seed=73, steps=2), wg_per_cu=1)


def _clip_segments():
    a = (2 * C + 4 + 3) // 4 * 4 + 1  # one element off alignment
    b = (a + 261 + 3) // 4 * 4
    return [(0, 2 * C + 4, True), (a, 261, True), (b, 7, False)]


@combos
def test_clipped(gpu, gdt, state):
    """The CLIP instances: norm pass over the set -> coefficient (< 1, a device scalar) -> update,
    grad_div = 3, coupled weight decay, over full chunks, a partial chunk, the scalar kernel and a
    segment without a gradient."""
    _check(gpu, _Case.random(gdt, state, _clip_segments(), seed=74, clip=True, div=3.0,
                             hp=dict(weight_decay=1e-2)))


@combos
def test_guarded(gpu, gdt, state):
    """The GUARD instances: with a finite coefficient the clipped run's bits (the oracle's); with a
    NaN coefficient p, m and v stay byte for byte."""
    from zero_amd.kernels import sr_keys

    case = _Case.random(gdt, state, _clip_segments(), seed=75, clip="fixed", div=3.0, steps=2)
    _check(gpu, case)
    _check(gpu, case, guard=True)
    T, G, aset = case.build(gpu)
    before = {k: v.clone() for k, v in T.items()}
    case.upload(G, case.grads[0])
    nan = torch.full((1,), float("nan"), device=gpu)
    for lf in (0, 1):
        _tune(b"adam_loads_first", lf)
        try:
            aset.run_psr(case.ahp(case.hps[0], 3.0), case.m_base(T), sr_keys(SEED, 1),
                         torch.cuda.current_stream(), coef=nan, guard=True)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
        for k in T:
            assert torch.equal(T[k], before[k]), (k, lf)


@combos
def test_set_grads_rebinding(gpu, gdt, state):
    """A set built without gradients, bound by zs_adamset_set_grads, one segment left at 0: it
    still decays (weight decay) and still rounds.  Then re-bound to a second buffer."""
    from zero_amd.kernels import sr_keys

    segs = [(0, C + 8, True), (C + 8, 2 * C + 3, False), (3 * C + 12, 300, True)]
    case = _Case.random(gdt, state, segs, seed=76, steps=2, hp=dict(weight_decay=0.1))
    want = case.reference()
    zero_seg = slice(C + 8, 3 * C + 11)
    assert (want["p"][zero_seg] != case.state0["p"][zero_seg]).mean() > 0.1
    T, G, aset = case.build(gpu, bind=False)
    G2 = torch.zeros_like(G)
    st = torch.cuda.current_stream()
    for h, g, buf in zip(case.hps, case.grads, (G, G2)):
        case.upload(buf, g)
        ptrs = [buf.data_ptr() + o * buf.element_size() if has_g else 0 for o, _, has_g in segs]
        aset.set_grads(np.array(ptrs, np.uint64), st)
        aset.run_psr(case.ahp(h, 1.0), case.m_base(T), sr_keys(SEED, h["step"]), st)
    torch.cuda.synchronize()
    got = case.download(T)
    for name, ref in want.items():
        assert np.array_equal(got[name], ref), name
    per = BYTES[(gdt, "f32" if state == "f32" else "bf16")]
    gsz = 4 if gdt == "fp32" else 2
    assert aset.bytes == per * (C + 8 + 300) + (per - gsz) * (2 * C + 3)


@combos
def test_special_values(gpu, gdt, state):
    """NaN, +Inf and -Inf in the gradient (a full chunk and the partial one) and in the parameter,
    denormal parameters, moments of the wide class (squares that overflow)."""
    n = sp.N
    s = sp.planted("wide", n + SLACK, seed=6)
    g = sp.special_grads(s, more=(2 * C + 1,))
    g = np.ascontiguousarray(g if gdt == "fp32" else zo.f32_to_bf16_bits(g))
    p0 = s["p"].copy()
    p0[[10, C + 10]] = np.nan
    p0[[11, C + 11]] = np.inf
    p0[[12, C + 12]] = -np.inf
    p0[20:40] = np.ldexp(np.float32(1.5), -130)  # denormal in bf16 too
    p0[2 * C + 2: 2 * C + 5] = [-np.ldexp(np.float32(1.0), -133), np.nan, np.inf]
    case = _Case(gdt, state, [(0, n, True)], [g], [{**sp.hp_of("wd")}], p0=p0, m0=s["m"], v0=s["v"])
    want = case.reference()
    assert (want["p"][[3, 10, C + 10, 2 * C + 1, 2 * C + 3]] == 0x7FC0).all()  # canon's NaN
    _check(gpu, case)


@pytest.mark.parametrize("gdt,state", [(g, s) for g in GDT for s in ("f32", "bf16")])
def test_bytes(gpu, gdt, state):
    n = 3 * C + 8
    case = _Case.random(gdt, state, [(0, n, True)], seed=1, steps=1)
    _, _, aset = case.build(gpu)
    assert aset.elems == n and aset.bytes == BYTES[(gdt, state)] * n


def test_refusals(gpu):
    """ZS_ERR_INVALID and nothing touched: the other run paths on a ZS_BF16_SR set, run_psr on a
    split set, amsgrad, guard without a coefficient, m below m_base or a fraction of an element from
    it; a seg with carry, vmax, master_out or another p_out; an SGD set."""
    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_BF16_SR, ZS_ERR_INVALID, ZS_F32, ZeroAmdError
    from zero_amd.kernels import AdamSet, SgdSet, adam_hparams, sr_keys

    n = 64
    p = torch.full((n,), 0x3F80, dtype=torch.int16, device=gpu)
    g = torch.full((n,), 0x3C00, dtype=torch.int16, device=gpu)
    lo, m, v = (torch.zeros(n, dtype=torch.int16, device=gpu) for _ in range(3))
    m32, v32, x = (torch.zeros(n, device=gpu) for _ in range(3))
    row = [g.data_ptr(), p.data_ptr(), 0, p.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 0, n]
    row32 = row[:4] + [m32.data_ptr(), v32.data_ptr(), 0, 0, n]
    mk = lambda r, sd=ZS_BF16, pd=ZS_BF16_SR: AdamSet(np.array([r], np.uint64), ZS_BF16, pd,  # noqa: E731
                                                     state_dtype=sd)
    st = torch.cuda.current_stream()
    coef = torch.ones(1, device=gpu)
    hp, keys = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1), sr_keys(0, 1)
    ams = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, amsgrad=True)

    def refused(fn):
        with pytest.raises(ZeroAmdError) as e:
            fn()
        assert e.value.code == ZS_ERR_INVALID

    for col, val in ((2, lo.data_ptr()), (6, x.data_ptr()), (7, x.data_ptr()), (3, lo.data_ptr()),
                     (3, 0)):
        bad = list(row)
        bad[col] = val
        refused(lambda: mk(bad))
    refused(lambda: SgdSet(np.array([row32[:5] + [0, 0, 0, n]], np.uint64), ZS_BF16, ZS_BF16_SR))
    refused(lambda: mk(row, sd=7))
    for aset, base in ((mk(row), m.data_ptr()), (mk(row32, sd=ZS_F32), m32.data_ptr())):
        refused(lambda: aset.run(hp, st))
        refused(lambda: aset.run_clipped(hp, coef, st))
        refused(lambda: aset.run_guarded(hp, coef, st))
        if aset.state_dtype == ZS_BF16:
            refused(lambda: aset.run_sr(hp, base, keys, st))
            refused(lambda: aset.run_sr(hp, base, keys, st, coef=coef, guard=True))
        refused(lambda: aset.run_psr(ams, base, keys, st))
        refused(lambda: aset.run_psr(hp, base, keys, st, guard=True))
        refused(lambda: aset.run_psr(hp, base + 2, keys, st))  # m below m_base
        refused(lambda: aset.run_psr(hp, base - 1, keys, st))  # a fraction of an element
    refused(lambda: mk(row32, sd=ZS_F32).run_psr(hp, m32.data_ptr() - 2, keys, st))  # half an fp32
    split = mk(row[:2] + [lo.data_ptr()] + row[3:], pd=ZS_BF16_SPLIT)
    refused(lambda: split.run_psr(hp, m.data_ptr(), keys, st))
    torch.cuda.synchronize()
    assert (p == 0x3F80).all() and not (m.any() or v.any() or lo.any() or m32.any() or v32.any())
    good = mk(row)
    good.run_psr(hp, m.data_ptr() - 2 * 7, keys, st)  # the same rows run, from a whole distance
    torch.cuda.synchronize()
    assert m.any() and v.any() and (p != 0x3F80).any()
