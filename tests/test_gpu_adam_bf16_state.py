"""The fused Adam kernels with bf16 moments (zs_adamset_create_ex, ZS_BF16 state), bit for bit
against the restatement of tests/_bf16_state_oracle.py: widen m and v, the unchanged C oracle step,
round m' and v' to nearest even.

The model is tests/test_gpu_adam_chunks.py: every array the kernel writes is compared whole (gaps
between segments and the slack behind the last one included), with ``adam_loads_first`` at 0 and at
1, against the oracle and against each other.  A NaN need only be a NaN.  Kinds (C: the chunk):

  split       split master, bf16 gradient                   C = 4096   18 B/element
  split_wide  split master, fp32 gradient                   C = 4096   20
  master      fp32 master with a bf16 p_out, bf16 gradient  C = 2048   20
  f32         fp32 parameters, fp32 gradient                C = 2048   20

A clipped run (zs_adamset_run_clipped) gets its coefficient from the set's own sum-of-squares pass
and zs_clip_coef on the device; the reference is the unchanged fp32 oracle step on the pre-clipped
gradient fl(fl(g / div) * coef) with the coefficient read back, as tests/test_gpu_gradnorm.py.
"""
import numpy as np
import pytest
import torch

import _adam_space as sp
import _bf16_state_oracle as bo
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_adam_chunks import SLACK, TIES, _mixed_table, _tune, scalar_table_past_the_grid

pytestmark = pytest.mark.gpu

KINDS = ("split", "split_wide", "master", "f32")
CHUNK = {"split": 4096, "split_wide": 4096, "master": 2048, "f32": 2048}
BYTES = {"split": 18, "split_wide": 20, "master": 20, "f32": 20}
SPLIT = ("split", "split_wide")
G32 = ("split_wide", "f32")
BETAS = dict(beta1=0.9, beta2=0.95)  # inside the guard (1 - beta >= 2^-8)
CLIP_COEF = np.float32(0.3)  # 0x3E99999A: no power of two, so g * coef rounds


def _hp(**kw):
    return {**sp.DEFAULT, **BETAS, **kw}


class _Case:
    """Segments (offset, n, has_grad) in one flat arena, an initial state, one gradient arena and
    one hyperparameter dict per step.  ``clip``: True — the coefficient of each step from the
    device's own norm pass — or "fixed": CLIP_COEF (gradients whose squares overflow fp32)."""

    def __init__(self, kind, segs, grads, hps, *, p0, m0=None, v0=None, clip=False, div=1.0):
        self.kind, self.segs, self.grads, self.hps = kind, segs, grads, hps
        self.clip, self.div = clip, float(div)
        self.N = N = max(o + n for o, n, _ in segs) + SLACK
        assert all(len(g) == N for g in grads) and len(p0) == N
        z = np.zeros(N, np.uint16)
        self.state0 = {"m": z.copy() if m0 is None else bo.narrow(m0),
                       "v": z.copy() if v0 is None else bo.narrow(v0)}
        if kind in SPLIT:
            self.state0["hi"], self.state0["lo"] = sp.split_master(p0)
        else:
            self.state0["p"] = np.ascontiguousarray(p0, np.float32)
            if kind == "master":
                self.state0["pb"] = np.zeros(N, np.uint16)

    @classmethod
    def random(cls, kind, segs, seed, steps=3, nan_at=(), hp=None, **kw):
        """Zero moments, a small random master with every tie class of the split encoding at the
        head of each segment and of its second chunk, ``steps`` random gradients."""
        rng = np.random.default_rng(seed)
        N = max(o + n for o, n, _ in segs) + SLACK
        p0 = (rng.standard_normal(N) * 0.02).astype(np.float32)
        u = p0.view(np.uint32)
        for o, n, _ in segs:
            for at in (o, o + CHUNK[kind]):
                k = max(0, min(len(TIES), o + n - at))
                u[at:at + k] = TIES[:k]
        grads = []
        for _ in range(steps):
            g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
            for at in nan_at:
                g[at] = np.nan
            grads.append(g if kind in G32 else zo.f32_to_bf16_bits(g))
        hps = [_hp(step=t, **(hp or {})) for t in range(1, steps + 1)]
        return cls(kind, segs, grads, hps, p0=p0, **kw)

    @staticmethod
    def canon(out):
        return {k: sp.canon(np.ascontiguousarray(a), out["hi"] if k == "lo" else None)
                for k, a in out.items()}

    # ---- the oracle, segment by segment, in place on slices of the arena ----
    def reference(self, coefs=None):
        kind = self.kind
        out = {k: a.copy() for k, a in self.state0.items()}
        for t, (hp, G) in enumerate(zip(self.hps, self.grads)):
            chp = c_oracle.hparams(grad_div=1.0 if self.clip else self.div, **hp)
            for o, n, has_g in self.segs:
                sl = slice(o, o + n)
                g = G[sl].copy()
                if not has_g:
                    g[:] = 0
                m, v = out["m"][sl], out["v"][sl]
                if self.clip:
                    gf = g if kind in G32 else zo.bf16_bits_to_f32(g)
                    with np.errstate(all="ignore"):
                        gp = np.ascontiguousarray((gf / np.float32(self.div)).astype(np.float32)
                                                  * np.float32(coefs[t]))
                    p = c_oracle.join_master(out["hi"][sl], out["lo"][sl]) if kind in SPLIT \
                        else out["p"][sl]
                    bo.adam_f32(p, gp, m, v, chp)
                    if kind in SPLIT:
                        out["hi"][sl], out["lo"][sl] = c_oracle.split_master(p)
                    elif kind == "master":
                        out["pb"][sl] = zo.f32_to_bf16_bits(p)
                elif kind == "split":
                    bo.adam_bf16_split(out["hi"][sl], out["lo"][sl], g, m, v, chp)
                elif kind == "split_wide":
                    bo.adam_f32grad_split(out["hi"][sl], out["lo"][sl], g, m, v, chp)
                elif kind == "master":
                    bo.adam_bf16(out["p"][sl], out["pb"][sl], g, m, v, chp)
                else:
                    bo.adam_f32(out["p"][sl], g, m, v, chp)
        return self.canon(out)

    # ---- the kernels ----
    def build(self, gpu):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import AdamSet

        kind = self.kind
        T = {k: torch.from_numpy(a.view(np.int16) if a.itemsize == 2 else a.copy()).to(gpu)
             for k, a in self.state0.items()}
        G = torch.zeros(self.N, dtype=torch.float32 if kind in G32 else torch.int16, device=gpu)
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in self.segs:
            g = G.data_ptr() + o * G.element_size() if has_g else 0
            if kind in SPLIT:
                row = [g, at("hi", o), at("lo", o), at("hi", o)]
            else:
                row = [g, at("p", o), at("p", o), at("pb", o)]
            rows.append(row + [at("m", o), at("v", o), 0, 0, n])
        aset = AdamSet(np.array(rows, dtype=np.uint64), ZS_F32 if kind in G32 else ZS_BF16,
                       ZS_BF16_SPLIT if kind in SPLIT else ZS_BF16, wide_grads=kind == "split_wide",
                       state_dtype=ZS_BF16)
        return T, G, aset

    def run_gpu(self, gpu, loads_first, wg_per_cu=0, max_norm=None):
        """(arrays, coefficients): the steps on the GPU; ``max_norm``: clipped, with the
        coefficient of each step from the device."""
        from zero_amd.kernels import adam_hparams, clip_coef, sqnorm_reduce

        T, G, aset = self.build(gpu)
        st = torch.cuda.current_stream()
        partials = torch.zeros(aset.sqnorm_partials + 8, dtype=torch.float64, device=gpu)
        sumsq, out2 = torch.zeros(1, device=gpu), torch.zeros(2, device=gpu)
        coefs = []
        _tune(b"adam_loads_first", loads_first)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            for h, g in zip(self.hps, self.grads):
                G.copy_(torch.from_numpy(g if self.kind in G32 else g.view(np.int16)))
                hp = adam_hparams(h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"],
                                  h["step"], decoupled=h["decoupled"], maximize=h["maximize"],
                                  grad_div=self.div)
                if self.clip == "fixed":
                    out2.copy_(torch.from_numpy(np.array([0.0, CLIP_COEF], np.float32)))
                    aset.run_clipped(hp, out2.data_ptr() + 4, st)
                    coefs.append(CLIP_COEF)
                elif self.clip:
                    aset.grad_sqnorm(partials, st)
                    sqnorm_reduce(partials, aset.sqnorm_partials, sumsq, st)
                    clip_coef(sumsq, self.div, max_norm, out2, st)
                    aset.run_clipped(hp, out2.data_ptr() + 4, st)
                    torch.cuda.synchronize()
                    coefs.append(np.float32(out2.cpu().numpy()[1]))
                else:
                    aset.run(hp, st)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        out = {k: v.cpu().numpy() for k, v in T.items()}
        return self.canon({k: a.view(np.uint16) if a.itemsize == 2 else a
                           for k, a in out.items()}), coefs

    def max_norm(self):
        """Half the L2 norm of the first step's averaged gradient: every step is clipped."""
        g = self.grads[0]
        x = (g if self.kind in G32 else zo.bf16_bits_to_f32(g)).astype(np.float64)
        ss = sum(float(np.sum(x[o:o + n] ** 2)) for o, n, has_g in self.segs if has_g)
        return 0.5 * np.sqrt(ss) / self.div


def _check(gpu, case, wg_per_cu=0):
    max_norm = case.max_norm() if case.clip is True else None
    got = {lf: case.run_gpu(gpu, lf, wg_per_cu, max_norm) for lf in (0, 1)}
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


def _lengths(C):
    return [4, C - 4, C, C + 4, 2 * C + 4, 3 * C - 4]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", range(6))
def test_boundary_lengths(gpu, kind, k):
    """One segment of n = 4, C-4, C, C+4, 2C+4, 3C-4, 3 steps from zero moments."""
    n = _lengths(CHUNK[kind])[k]
    _check(gpu, _Case.random(kind, [(0, n, True)], seed=200 + k))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wg_per_cu", [1, 0])
def test_mixed_table(gpu, kind, wg_per_cu):
    """tests/test_gpu_adam_chunks.py's mixed table — a segment without a gradient, one that is one
    element off alignment, a partial last chunk — with one workgroup per CU (every workgroup loops
    over several chunks and segments) and at the default grid."""
    segs = _mixed_table(CHUNK[kind])
    if wg_per_cu:
        chunks = sum(n // CHUNK[kind] for _, n, _ in segs)
        assert 2 * wg_per_cu * torch.cuda.get_device_properties(gpu).multi_processor_count <= chunks
    _check(gpu, _Case.random(kind, segs, seed=9), wg_per_cu)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_scalar_table_strides_past_the_grid(gpu, kind, clip):
    """The scalar instance with one workgroup per CU over more than 2 * cus chunks of 256."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    segs, sca_chunks = scalar_table_past_the_grid(cus)
    assert sca_chunks == 2 * cus + 8
    _check(gpu, _Case.random(kind, segs, seed=33, clip=clip, div=3.0 if clip else 1.0),
           wg_per_cu=1)


def _space_case(kind, cls, hp, special=False, clip=False):
    """One step from a planted state, one segment of N = 8192 + 5 elements: full chunks, a partial
    one and a one-element scalar tail."""
    n = sp.N
    s = sp.planted(cls, n + SLACK, seed=6)
    g = sp.special_grads(s, more=(2 * CHUNK[kind] + 1,)) if special else s["g"]
    g = np.ascontiguousarray(g if kind in G32 else zo.f32_to_bf16_bits(g))
    return _Case(kind, [(0, n, True)], [g], [dict(hp)], p0=s["p"], m0=s["m"], v0=s["v"],
                 clip=clip, div=3.0 if clip else 1.0)


POINTS = [k for k, v in sp.GRID.items() if not v.get("amsgrad")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", POINTS)
def test_grid(gpu, point, cls, kind):
    """Every grid point without amsgrad, both magnitude classes (the wide one: moments past the
    largest bf16 round to Inf, squares that overflow, denormals)."""
    _check(gpu, _space_case(kind, cls, sp.hp_of(point)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", sp.CLASSES)
def test_special_gradients(gpu, cls, kind):
    """NaN, +Inf and -Inf gradients in a full chunk and in the partial one."""
    case = _space_case(kind, cls, sp.hp_of("wd"), special=True)
    want = case.reference()
    assert (want["m"][[3, 2 * CHUNK[kind] + 1]] == 0x7FC0).all()  # canon's NaN
    _check(gpu, case)


@pytest.mark.parametrize("kind", KINDS)
def test_clipped(gpu, kind):
    """The CLIP twin: 3 steps of norm -> coefficient -> clipped update over full chunks, a partial
    chunk, the scalar kernel and a segment without a gradient, grad_div = 3, weight decay."""
    C = CHUNK[kind]
    a = (2 * C + 4 + 3) // 4 * 4 + 1  # one element off alignment
    b = (a + 261 + 3) // 4 * 4
    segs = [(0, 2 * C + 4, True), (a, 261, True), (b, 7, False)]
    _check(gpu, _Case.random(kind, segs, seed=41, clip=True, div=3.0, hp=dict(weight_decay=1e-2)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", sp.CLASSES)
def test_clipped_planted(gpu, cls, kind):
    """The CLIP twin from a planted state with a coefficient that is no power of two, under the
    high lerp form and AdamW."""
    hp = {**sp.hp_of("adamw"), "beta1": 0.3}
    _check(gpu, _space_case(kind, cls, hp, clip="fixed"))


@pytest.mark.parametrize("kind", KINDS)
def test_bytes(gpu, kind):
    n = 3 * CHUNK[kind] + 8
    case = _Case.random(kind, [(0, n, True)], seed=1, steps=1)
    _, _, aset = case.build(gpu)
    assert aset.elems == n and aset.bytes == BYTES[kind] * n


def test_refusals(gpu):
    """ZS_ERR_INVALID: a segment with vmax, one with carry, a run with amsgrad."""
    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_ERR_INVALID, ZeroAmdError
    from zero_amd.kernels import AdamSet, SgdSet, adam_hparams

    n = 64
    h = torch.zeros(n, dtype=torch.int16, device=gpu)
    lo, g, m, v = (torch.zeros_like(h) for _ in range(4))
    x = torch.zeros(n, device=gpu)
    row = [g.data_ptr(), h.data_ptr(), lo.data_ptr(), h.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 0, n]
    mk = lambda r, **kw: AdamSet(np.array([r], np.uint64), ZS_BF16, ZS_BF16_SPLIT, **kw)  # noqa: E731
    for col in (6, 7):  # vmax, carry
        bad = list(row)
        bad[col] = x.data_ptr()
        with pytest.raises(ZeroAmdError) as e:
            mk(bad, state_dtype=ZS_BF16)
        assert e.value.code == ZS_ERR_INVALID
    with pytest.raises(ZeroAmdError) as e:
        mk(row, state_dtype=7)
    assert e.value.code == ZS_ERR_INVALID
    with pytest.raises(ZeroAmdError) as e:
        SgdSet(np.array([row[:5] + [0, 0, 0, n]], np.uint64), ZS_BF16, ZS_BF16_SPLIT,
               state_dtype=ZS_BF16)
    assert e.value.code == ZS_ERR_INVALID
    aset = mk(row, state_dtype=ZS_BF16)
    st = torch.cuda.current_stream()
    coef = torch.ones(1, device=gpu)
    ams = adam_hparams(1e-3, 0.9, 0.95, 1e-8, 0.0, 1, amsgrad=True)
    with pytest.raises(ZeroAmdError) as e:
        aset.run(ams, st)
    assert e.value.code == ZS_ERR_INVALID
    with pytest.raises(ZeroAmdError) as e:
        aset.run_clipped(ams, coef, st)
    assert e.value.code == ZS_ERR_INVALID
    aset.run(adam_hparams(1e-3, 0.9, 0.95, 1e-8, 0.0, 1), st)  # the same set runs without it
    torch.cuda.synchronize()
    assert not m.any() and not v.any() and not h.any()  # (a zero gradient on a zero state)
