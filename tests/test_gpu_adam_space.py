"""The fused Adam kernels over the hyperparameter and magnitude space of tests/_adam_space.py,
bit for bit against the C oracle (which tests/test_adam_oracle.py pins to live torch).

One step from a planted non-zero m, v, vmax (and carry), per grid point, magnitude class and kind,
over one table that reaches every kernel path (C = 4,096 elements for the split master, 2,048
otherwise):
  (0, 2C+4, gradient)   full chunks (the loads-first body) and a partial chunk (the predicated one)
  one element off alignment, n = 261, gradient: the scalar kernel, two workgroups
  aligned, n = 7, no gradient: the vector kernel's first 4 and a 3-element scalar tail
Built on tests/test_gpu_adam_chunks.py: the arrays are compared whole (gaps and the slack behind
the last segment included), with ``adam_loads_first`` at 0 and at 1.  A NaN need only be a NaN.
Under 15k elements per case.
"""
import numpy as np
import pytest
import torch

import _adam_space as sp
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_adam_chunks import CHUNK, KINDS, SLACK, _Case, _check, _tune

pytestmark = pytest.mark.gpu

CLIP_COEF = np.float32(0.3)  # 0x3E99999A: no power of two, so g * coef rounds


def _table(C):
    a = (2 * C + 4 + 3) // 4 * 4 + 1  # one element off 16-byte alignment
    b = (a + 261 + 3) // 4 * 4
    return [(0, 2 * C + 4, True), (a, 261, True), (b, 7, False)]


class _SpaceCase(_Case):
    """One step from a planted state with the hyperparameters of one grid point."""

    def __init__(self, kind, cls, hp, *, carry=False, clip=False, special=False, seed=5):
        self.kind, self.ams, self.carry, self.clip = kind, bool(hp["amsgrad"]), carry, clip
        self.hp = dict(hp)
        if carry:
            self.hp.update(grad_div=3.0, carry_mul=2.0)
        elif clip:
            self.hp.update(grad_div=3.0)
        self.segs = _table(CHUNK[kind])
        self.N = N = max(o + n for o, n, _ in self.segs) + SLACK
        assert N - SLACK < 15000
        s = sp.planted(cls, N, seed)
        # specials in a full chunk, in the partial chunk and in the scalar kernel's second workgroup
        self.special_at = (3, 2 * CHUNK[kind], self.segs[1][0] + 257)
        g = sp.special_grads(s, more=self.special_at[1:]) if special else s["g"]
        self.g = g if kind == "f32" else zo.f32_to_bf16_bits(g)
        self.state0 = {k: s[k] for k in ("m", "v")}
        if self.ams:
            self.state0["vmax"] = s["vmax"]
        if carry:
            self.state0["carry"] = s["carry"]
        if kind == "split":
            self.state0["hi"], self.state0["lo"] = sp.split_master(s["p"])
        else:
            self.state0["p"] = s["p"]
            if kind == "bf16":
                self.state0["pb"] = np.zeros(N, np.uint16)

    @staticmethod
    def _canon(out):
        return {k: sp.canon(np.ascontiguousarray(a), out["hi"] if k == "lo" else None).view(
            np.float32 if a.itemsize == 4 else np.uint16) for k, a in out.items()}

    # ---- the C oracle, segment by segment, in place on slices of the arena ----
    def reference(self):
        kind = self.kind
        out = {k: a.copy() for k, a in self.state0.items()}
        hp = dict(self.hp)
        if self.clip:  # the unmodified oracle on the pre-clipped gradient fl(fl(g / div) * coef)
            div = np.float32(hp.pop("grad_div"))
        chp = c_oracle.hparams(**hp)
        for o, n, has_g in self.segs:
            sl = slice(o, o + n)
            g = self.g[sl].copy()
            if not has_g:
                g[:] = 0
            opt = dict(vmax=out["vmax"][sl] if self.ams else None,
                       carry=out["carry"][sl] if self.carry else None)
            if self.clip:
                gf = g if kind == "f32" else zo.bf16_bits_to_f32(g)
                with np.errstate(all="ignore"):
                    gp = np.ascontiguousarray((gf / div).astype(np.float32) * CLIP_COEF)
                p = c_oracle.join_master(out["hi"][sl], out["lo"][sl]) if kind == "split" \
                    else out["p"][sl]
                c_oracle.adam_f32(p, gp, out["m"][sl], out["v"][sl], chp, **opt)
                if kind == "split":
                    out["hi"][sl], out["lo"][sl] = c_oracle.split_master(p)
                elif kind == "bf16":
                    out["pb"][sl] = zo.f32_to_bf16_bits(p)
            elif kind == "split":
                c_oracle.adam_bf16_split(out["hi"][sl], out["lo"][sl], g, out["m"][sl],
                                         out["v"][sl], chp, **opt)
            elif kind == "bf16":
                c_oracle.adam_bf16(out["p"][sl], out["pb"][sl], g, out["m"][sl], out["v"][sl],
                                   chp, **opt)
            else:
                c_oracle.adam_f32(out["p"][sl], g, out["m"][sl], out["v"][sl], chp, **opt)
        return self._canon(out)

    # ---- the kernels ----
    def run_gpu(self, gpu, loads_first, wg_per_cu=0):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import AdamSet, adam_hparams

        kind = self.kind
        T = {k: torch.from_numpy(a.view(np.int16) if a.itemsize == 2 else a.copy()).to(gpu)
             for k, a in self.state0.items()}
        G = torch.from_numpy(self.g if kind == "f32" else self.g.view(np.int16)).to(gpu)
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in self.segs:
            g = G.data_ptr() + o * G.element_size() if has_g else 0
            if kind == "split":
                row = [g, at("hi", o), at("lo", o), at("hi", o)]
            else:
                row = [g, at("p", o), at("p", o), at("pb", o)]
            rows.append(row + [at("m", o), at("v", o), at("vmax", o), at("carry", o), n])
        aset = AdamSet(np.array(rows, dtype=np.uint64), ZS_F32 if kind == "f32" else ZS_BF16,
                       ZS_BF16_SPLIT if kind == "split" else ZS_BF16)
        h = self.hp
        hp = adam_hparams(h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["step"],
                          decoupled=h["decoupled"], amsgrad=h["amsgrad"], maximize=h["maximize"],
                          grad_div=h.get("grad_div", 1.0), carry_mul=h.get("carry_mul", 0.0))
        coef = torch.from_numpy(np.array([CLIP_COEF])).to(gpu)
        st = torch.cuda.current_stream()
        _tune(b"adam_loads_first", loads_first)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            if self.clip:
                aset.run_clipped(hp, coef, st)
            else:
                aset.run(hp, st)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        out = {k: v.cpu().numpy() for k, v in T.items()}
        return self._canon({k: a.view(np.uint16) if a.itemsize == 2 else a for k, a in out.items()})


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", list(sp.GRID))
def test_grid(gpu, point, cls, kind):
    _check(gpu, _SpaceCase(kind, cls, sp.hp_of(point)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", ["default", "all_adamw", "b1_0.3"])
def test_carry(gpu, point, cls, kind):
    """grad_div = 3 with carry_mul = 2: the CARRY instances, the carry array compared as well."""
    _check(gpu, _SpaceCase(kind, cls, sp.hp_of(point), carry=True))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", sp.CLASSES)
def test_clipped(gpu, cls, kind):
    """zs_adamset_run_clipped with a coefficient that is no power of two (0.3 in fp32) and
    grad_div = 3, under the high lerp form, weight decay and amsgrad."""
    hp = {**sp.hp_of("all_adam"), "beta1": 0.3}
    _check(gpu, _SpaceCase(kind, cls, hp, clip=True))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", ["amsgrad", "all_adamw"])
def test_nan_inf_amsgrad(gpu, point, cls, kind):
    """NaN, +Inf and -Inf gradient elements under amsgrad, in a full chunk, in the partial chunk
    and in the scalar kernel: vmax is NaN where exp_avg_sq is."""
    case = _SpaceCase(kind, cls, sp.hp_of(point), special=True)
    want = case.reference()
    nan = list(case.special_at)
    assert np.isnan(want["vmax"][nan]).all() and np.isnan(want["v"][nan]).all()
    _check(gpu, case)
