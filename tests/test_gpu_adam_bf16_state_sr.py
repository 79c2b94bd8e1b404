"""The fused Adam kernels with bf16 moments stored with stochastic rounding (zs_adamset_run_sr), bit
for bit on every element of p / hi / lo / m / v against the restatement of
tests/_bf16_state_sr_oracle.py, at torch's default betas (0.9, 0.999).

The cases are tests/test_gpu_adam_bf16_state.py's (same kinds, same arrays, whole-arena
comparison, ``adam_loads_first`` at 0 and at 1 against the oracle and against each other) with the
generator's inputs added: a seed, each step's keys from (seed, step), and ``m_base`` = the address of
the m arena less ``2 * shift`` bytes, so the element at arena offset o has index ``shift + o``.
``m_base`` is only subtracted from, so a shift of 2^32 - 5000 puts the carry into the high word of
the index inside the first segment on a few kilobytes.
"""
import numpy as np
import pytest
import torch

import _adam_space as sp
import _bf16_state_sr_oracle as so
import test_gpu_adam_bf16_state as nb
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_adam_chunks import _mixed_table, _tune

pytestmark = pytest.mark.gpu

KINDS, CHUNK, SPLIT, G32 = nb.KINDS, nb.CHUNK, nb.SPLIT, nb.G32
BETAS = dict(beta1=0.9, beta2=0.999)  # torch's default: refused when rounding to nearest
SEED = (0xC0FFEE << 32) | 0x1234567


class _SrCase(nb._Case):
    seed, shift = SEED, 0

    @classmethod
    def random(cls, kind, segs, seed, *, shift=0, sr_seed=SEED, hp=None, **kw):
        case = super().random(kind, segs, seed, hp={**BETAS, **(hp or {})}, **kw)
        case.shift, case.seed = int(shift), int(sr_seed)
        return case

    def reference(self, coefs=None):
        kind = self.kind
        out = {k: a.copy() for k, a in self.state0.items()}
        for t, (hp, G) in enumerate(zip(self.hps, self.grads)):
            chp = c_oracle.hparams(grad_div=1.0 if self.clip else self.div, **hp)
            keys = so.keys_of(self.seed, hp["step"])
            for o, n, has_g in self.segs:
                sl = slice(o, o + n)
                e = np.arange(n, dtype=np.uint64) + np.uint64(self.shift + o)
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
                    so.adam_f32(p, gp, m, v, chp, e, keys)
                    if kind in SPLIT:
                        out["hi"][sl], out["lo"][sl] = c_oracle.split_master(p)
                    elif kind == "master":
                        out["pb"][sl] = zo.f32_to_bf16_bits(p)
                elif kind == "split":
                    so.adam_bf16_split(out["hi"][sl], out["lo"][sl], g, m, v, chp, e, keys)
                elif kind == "split_wide":
                    so.adam_f32grad_split(out["hi"][sl], out["lo"][sl], g, m, v, chp, e, keys)
                elif kind == "master":
                    so.adam_bf16(out["p"][sl], out["pb"][sl], g, m, v, chp, e, keys)
                else:
                    so.adam_f32(out["p"][sl], g, m, v, chp, e, keys)
        return self.canon(out)

    def run_gpu(self, gpu, loads_first, wg_per_cu=0, max_norm=None):
        from zero_amd.kernels import adam_hparams, clip_coef, sqnorm_reduce, sr_keys

        T, G, aset = self.build(gpu)
        m_base = T["m"].data_ptr() - 2 * self.shift
        assert m_base > 0
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
                keys = sr_keys(self.seed, h["step"])
                if self.clip:
                    aset.grad_sqnorm(partials, st)
                    sqnorm_reduce(partials, aset.sqnorm_partials, sumsq, st)
                    clip_coef(sumsq, self.div, max_norm, out2, st)
                    aset.run_sr(hp, m_base, keys, st, coef=out2.data_ptr() + 4)
                    torch.cuda.synchronize()
                    coefs.append(np.float32(out2.cpu().numpy()[1]))
                else:
                    aset.run_sr(hp, m_base, keys, st)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        out = {k: v.cpu().numpy() for k, v in T.items()}
        return self.canon({k: a.view(np.uint16) if a.itemsize == 2 else a
                           for k, a in out.items()}), coefs


def _four_segments(C):
    """Two full chunks + a predicated partial chunk + a 3-element scalar tail; one chunk exactly;
    5 elements; a segment one element off alignment (scalar throughout, two scalar chunks)."""
    segs, off = [], 0
    for n, shift in ((2 * C + 4 * 300 + 3, 0), (C, 0), (5, 0), (300, 1)):
        off = (off + 3) // 4 * 4 + shift
        segs.append((off, n, True))
        off += n
    return segs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_four_segments(gpu, kind, clip):
    """Every instance — {bf16, fp32} gradient x {split, not} x {plain, CLIP} x both
    ``adam_loads_first`` settings, and the scalar kernel — over three steps keyed 1 to 3."""
    case = _SrCase.random(kind, _four_segments(CHUNK[kind]), seed=61, clip=clip,
                          div=3.0 if clip else 1.0)
    assert [h["step"] for h in case.hps] == [1, 2, 3] and case.hps[0]["beta2"] == 0.999
    nb._check(gpu, case)
    if not clip:  # the draws matter: the moments differ from the ones rounded to nearest
        assert (nb._Case.reference(case)["v"] != case.reference()["v"]).mean() > 0.1


@pytest.mark.parametrize("kind", KINDS)
def test_index_crosses_2_to_the_32(gpu, kind):
    """m_base 2 * (2^32 - 5000) bytes below the arena: the index passes 2^32 inside the first
    segment (C = 4096: in its second full chunk; C = 2048: in the predicated partial one), and
    every later element carries a high word of 1."""
    C = CHUNK[kind]
    assert 5000 < _four_segments(C)[0][1]
    case = _SrCase.random(kind, _four_segments(C), seed=62, shift=(1 << 32) - 5000)
    low = _SrCase.random(kind, _four_segments(C), seed=62, shift=0)
    nb._check(gpu, case)
    assert (case.reference()["m"] != low.reference()["m"]).mean() > 0.1  # other draws


@pytest.mark.parametrize("kind", ["split", "f32"])
def test_several_chunks_per_workgroup(gpu, kind):
    """tests/test_gpu_adam_chunks.py's mixed table with one workgroup per CU: every workgroup
    loops over several chunks and segments, and the indices do not depend on the grid."""
    segs = _mixed_table(CHUNK[kind])
    chunks = sum(n // CHUNK[kind] for _, n, _ in segs)
    assert 2 * torch.cuda.get_device_properties(gpu).multi_processor_count <= chunks
    nb._check(gpu, _SrCase.random(kind, segs, seed=63, steps=2), wg_per_cu=1)


def test_special_values(gpu):
    """NaN and Inf gradients and moments past the largest bf16: a NaN moment is stored as a NaN,
    Inf as Inf, a finite value past the edge as the edge or Inf by its draw."""
    kind = "split"
    n = sp.N
    s = sp.planted("wide", n + nb.SLACK, seed=6)
    g = np.ascontiguousarray(zo.f32_to_bf16_bits(sp.special_grads(s, more=(2 * CHUNK[kind] + 1,))))
    case = _SrCase(kind, [(0, n, True)], [g], [{**sp.hp_of("wd"), **BETAS}], p0=s["p"], m0=s["m"],
                   v0=s["v"])
    want = case.reference()
    assert (want["m"][[3, 2 * CHUNK[kind] + 1]] == 0x7FC0).all()  # canon's NaN
    nb._check(gpu, case)


def test_refusals(gpu):
    """ZS_ERR_INVALID, nothing launched: an fp32-state set, amsgrad, m below m_base, an odd byte
    distance, an SGD set."""
    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_ERR_INVALID, ZeroAmdError
    from zero_amd.kernels import AdamSet, SgdSet, adam_hparams, sr_keys

    n = 64
    h = torch.zeros(n, dtype=torch.int16, device=gpu)
    lo, g, m, v = (torch.zeros_like(h) for _ in range(4))
    m32, v32 = torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    g.fill_(0x3C00)
    row = [g.data_ptr(), h.data_ptr(), lo.data_ptr(), h.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 0, n]
    row32 = row[:4] + [m32.data_ptr(), v32.data_ptr(), 0, 0, n]
    mk = lambda r, **kw: AdamSet(np.array([r], np.uint64), ZS_BF16, ZS_BF16_SPLIT, **kw)  # noqa: E731
    st = torch.cuda.current_stream()
    hp, keys = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1), sr_keys(0, 1)
    bad = [
        (mk(row32), hp, m32.data_ptr()),                                       # fp32 state
        (mk(row, state_dtype=ZS_BF16), adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, amsgrad=True),
         m.data_ptr()),                                                        # amsgrad
        (mk(row, state_dtype=ZS_BF16), hp, m.data_ptr() + 2),                  # m below m_base
        (mk(row, state_dtype=ZS_BF16), hp, m.data_ptr() - 1),                  # odd distance
        (SgdSet(np.array([row32[:5] + [0, 0, 0, n]], np.uint64), ZS_BF16, ZS_BF16_SPLIT),
         hp, m32.data_ptr()),                                                  # an SGD set
    ]
    for aset, hpx, base in bad:
        with pytest.raises(ZeroAmdError) as e:
            aset.run_sr(hpx, base, keys, st)
        assert e.value.code == ZS_ERR_INVALID
    torch.cuda.synchronize()
    assert not m.any() and not v.any() and not h.any() and not m32.any()  # nothing ran
    good = mk(row, state_dtype=ZS_BF16)
    good.run_sr(hp, m.data_ptr() - 2 * 7, keys, st)  # the same set runs from an even distance
    torch.cuda.synchronize()
    assert m.any() and v.any()
