"""The fused SGD kernels over the hyperparameter and magnitude space of tests/_sgd_space.py, bit for
bit against tests/_sgd_oracle.py (which tests/test_sgd_oracle.py pins to live torch over the same
space).

One step from a planted parameter, momentum buffer (and carry), per grid point, magnitude class and
kind, over one table that reaches every kernel path (C = 4,096 elements for a split master, 2,048
otherwise):
  (0, 2C+4, gradient)   full chunks (the loads-first body) and a partial chunk (the predicated one)
  one element off alignment, n = 261, gradient: the scalar kernel, two workgroups
  aligned, n = 7, no gradient: the vector kernel's first 4 and a 3-element scalar tail, g = 0
Built on tests/test_gpu_sgd_kernel.py: the arrays are compared whole (gaps and the slack behind the
last segment included), with ``adam_loads_first`` at 0 and at 1.  A NaN need only be a NaN, and the
residual of a NaN split master reads 0.  Under 15k elements per case.

Kinds: ``split`` (bf16 gradient, split master), ``bf16`` (bf16 gradient, fp32 master and its bf16
copy), ``f32`` (fp32 gradient and parameter) and ``f32split`` (fp32 gradient over the split master,
ZeRO-3 after an fp32-accumulated step; reference: tests/_accum32_oracle.py's join, fp32 update,
split).  The library has no carry instance of ``f32split`` and refuses one when the set is made
(ZeRO-1, the carry's only user, never has such a set): test_carry runs the other three, and
test_carry_over_f32split_is_refused holds the refusal.
"""
import numpy as np
import pytest
import torch

import _accum32_oracle as a32
import _sgd_oracle as so
import _sgd_space as ss
from test_gpu_sgd_kernel import CHUNK, SLACK, _Case, _check, _layout, _tune

pytestmark = pytest.mark.gpu

KINDS = ("split", "bf16", "f32", "f32split")
CHUNK_OF = dict(CHUNK, f32split=CHUNK["split"])
CLIP_COEF = np.float32(0.3)  # 0x3E99999A: no power of two, so g * coef rounds


def _table(C):
    return _layout([(2 * C + 4, True, 0), (261, True, 1), (7, False, 0)])


class _SpaceCase(_Case):
    """One step from a planted state with the hyperparameters of one grid point.  ``buffers``: the
    set has momentum buffers (default: the point has a momentum)."""

    def __init__(self, kind, cls, point, *, first=False, buffers=None, carry=None, clip=False,
                 special=False, seed=5):
        self.kind, self.first, self.clip = kind, first, clip
        self.carry = carry is not None
        self.hp = dict(ss.GRID[point])
        if carry is not None:
            self.hp.update(grad_div=carry[0], carry_mul=carry[1])
        elif clip:
            self.hp.update(grad_div=3.0)
        self.buffers = ss.has_momentum(point) if buffers is None else buffers
        self.split = kind in ("split", "f32split")
        self.wide_g = kind in ("f32", "f32split")
        C = CHUNK_OF[kind]
        self.segs = _table(C)
        assert self.segs[1][0] % 4 == 1 and self.segs[2][0] % 4 == 0
        self.N = N = max(o + n for o, n, _ in self.segs) + SLACK
        assert N - SLACK < 15000
        s = ss.planted(cls, N, seed)
        # specials in a full chunk, in the partial chunk and in the scalar kernel's second workgroup
        self.special_at = (3, 2 * C, self.segs[1][0] + 257)
        g = ss.special_grads(s, more=self.special_at[1:]) if special else s["g"]
        self.g = g.copy() if self.wide_g else so.f32_to_bf16_bits(g)
        self.state0 = {}
        if self.buffers:
            self.state0["buf"] = s["buf"]  # stale on a first step: it must not be read
        if self.carry:
            self.state0["carry"] = s["carry"]
        if self.split:
            self.state0["hi"], self.state0["lo"] = ss.split_master(s["p"])
        else:
            self.state0["p"] = s["p"]
            if kind == "bf16":
                self.state0["pb"] = np.zeros(N, np.uint16)

    @staticmethod
    def _canon(out):
        return {k: ss.canon(np.ascontiguousarray(a), out["hi"] if k == "lo" else None).view(
            np.float32 if a.itemsize == 4 else np.uint16) for k, a in out.items()}

    def param(self, out):
        """The fp32 parameter of a result of ``reference`` / ``run_gpu``."""
        return ss.join_master(out["hi"], out["lo"]) if self.split else out["p"]

    # ---- the numpy restatement, segment by segment on slices of the arena ----
    def reference(self):
        kind = self.kind
        out = {k: a.copy() for k, a in self.state0.items()}
        hp = so.SgdHP(first=self.first, **self.hp)
        use_buf = self.buffers and self.hp.get("momentum", 0.0) != 0
        coef = CLIP_COEF if self.clip else None
        for o, n, has_g in self.segs:
            sl = slice(o, o + n)
            g = self.g[sl].copy()
            if not has_g:
                g[:] = 0
            buf = out["buf"][sl] if use_buf else None
            cr = None
            kw = dict(carry=out["carry"][sl] if self.carry else None, coef=coef)
            if kind == "split":
                out["hi"][sl], out["lo"][sl], buf, cr = so.step_split(out["hi"][sl], out["lo"][sl],
                                                                     g, buf, hp, **kw)
            elif kind == "bf16":
                out["p"][sl], out["pb"][sl], buf, cr = so.step_bf16(out["p"][sl], g, buf, hp, **kw)
            elif kind == "f32":
                out["p"][sl], buf, cr = so.step_f32(out["p"][sl], g, buf, hp, **kw)
            else:
                assert not self.carry
                out["hi"][sl], out["lo"][sl], buf = a32.sgd_f32grad_split(
                    out["hi"][sl], out["lo"][sl], g, buf, hp, coef=coef)
            if use_buf:
                out["buf"][sl] = buf
            if self.carry:
                out["carry"][sl] = cr
        return self._canon(out)

    # ---- the kernels ----
    def run_gpu(self, gpu, loads_first=1, wg_per_cu=0):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import SgdSet, sgd_hparams

        T = {k: torch.from_numpy(a.view(np.int16) if a.itemsize == 2 else a.copy()).to(gpu)
             for k, a in self.state0.items()}
        G = torch.from_numpy(self.g if self.wide_g else self.g.view(np.int16)).to(gpu)
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in self.segs:
            assert 0 <= o and o + n <= self.N - SLACK  # every segment inside the arrays
            g = G.data_ptr() + o * G.element_size() if has_g else 0
            if self.split:
                row = [g, at("hi", o), at("lo", o), at("hi", o)]
            else:
                row = [g, at("p", o), at("p", o), at("pb", o)]
            rows.append(row + [at("buf", o), 0, 0, at("carry", o), n])
        sset = SgdSet(np.array(rows, dtype=np.uint64), ZS_F32 if self.wide_g else ZS_BF16,
                      ZS_BF16_SPLIT if self.split else ZS_BF16, wide_grads=self.kind == "f32split")
        hp = sgd_hparams(first=self.first, **self.hp)
        coef = torch.from_numpy(np.array([CLIP_COEF])).to(gpu) if self.clip else None
        st = torch.cuda.current_stream()
        _tune(b"adam_loads_first", loads_first)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            sset.run(hp, st, coef=coef)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        out = {k: v.cpu().numpy() for k, v in T.items()}
        return self._canon({k: a.view(np.uint16) if a.itemsize == 2 else a for k, a in out.items()})


def _bits(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint16)


def _each_kind(gpu, make, kinds=KINDS, after=None):
    """``_check`` on ``make(kind)`` for every kind, then ``after(case, want, got)``.  Every kind
    runs whatever the ones before it gave, and the test fails with all their differences.  (The
    kinds share one test item: one kind's part of the body takes a few milliseconds, the suite's
    collection of garbage after every item many times that.)"""
    failed = []
    for kind in kinds:
        case = make(kind)
        try:
            want, got = _check(gpu, case)
            if after is not None:
                after(case, want, got)
        except AssertionError as e:
            failed.append(f"{kind}: {e}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("cls", ss.CLASSES)
@pytest.mark.parametrize("point", list(ss.GRID))
def test_grid(gpu, point, cls):
    """Every grid point from the planted buffer, every kind.  A point without momentum has no
    buffer at all."""
    def make(kind):
        case = _SpaceCase(kind, cls, point)
        assert ("buf" in case.state0) == ss.has_momentum(point)
        return case

    _each_kind(gpu, make)


@pytest.mark.parametrize("cls", ss.CLASSES)
@pytest.mark.parametrize("point", ss.FIRST_POINTS)
def test_first_step(gpu, point, cls):
    """``first``: the device buffer holds the stale planted values and comes back as the step's
    gradient term (the oracle's first branch, which never reads it), whatever they were."""
    def moved(case, want, got):
        inside = np.zeros(case.N, bool)
        for o, n, _ in case.segs:
            inside[o:o + n] = True
        assert (_bits(want["buf"])[inside] != ss.canon(case.state0["buf"])[inside]).mean() > 0.9

    _each_kind(gpu, lambda kind: _SpaceCase(kind, cls, point, first=True), after=moved)


@pytest.mark.parametrize("cls", ["wide", "small"])
@pytest.mark.parametrize("point", ["mom0", "wd_big"])
def test_momentum_zero_keeps_wide_buffer(gpu, point, cls):
    """A set that has buffers, run without momentum: torch makes no buffer then, and the planted
    one (denormals, 2^61, exact zeros) stays bit for bit."""
    def kept(case, want, got):  # no NaN planted: canon changes nothing
        assert np.array_equal(_bits(got["buf"]), _bits(case.state0["buf"]))

    _each_kind(gpu, lambda kind: _SpaceCase(kind, cls, point, buffers=True), after=kept)


@pytest.mark.parametrize("cls", ss.CLASSES)
@pytest.mark.parametrize("div,mul", [(3.0, 2.0), (2.0, 1.0)])
@pytest.mark.parametrize("point", ["mom0.9", "nesterov_wd_max", "mom0"])
def test_carry(gpu, point, div, mul, cls):
    """The ZeRO-1 carry with a true division (3) and a reciprocal multiply (2): the CARRY
    instances of the three kinds that have one, the carry array compared as well."""
    def moved(case, want, got):
        assert (_bits(want["carry"]) != ss.canon(case.state0["carry"])).mean() > 0.5

    _each_kind(gpu, lambda kind: _SpaceCase(kind, cls, point, carry=(div, mul)), KINDS[:3], moved)


def test_carry_over_f32split_is_refused(gpu):
    """``f32split`` has no CARRY instance: the set is refused when it is made, whatever the point,
    class and divisor, so test_carry cannot run it."""
    from zero_amd._lib import ZS_ERR_INVALID, ZeroAmdError

    assert KINDS[3:] == ("f32split",)
    with pytest.raises(ZeroAmdError, match="takes no carry") as e:
        _SpaceCase("f32split", "normal", "mom0.9", carry=(3.0, 2.0)).run_gpu(gpu)
    assert e.value.code == ZS_ERR_INVALID


@pytest.mark.parametrize("cls", ss.CLASSES)
@pytest.mark.parametrize("point", ["all", "mom0"])
def test_clipped(gpu, point, cls):
    """The coefficient 0.3 (no power of two) read from device memory, with grad_div = 3."""
    _each_kind(gpu, lambda kind: _SpaceCase(kind, cls, point, clip=True))


@pytest.mark.parametrize("cls", ss.CLASSES)
@pytest.mark.parametrize("point", ["mom0.9", "nesterov_wd_max", "damp1", "lr_0"])
def test_nan_inf(gpu, point, cls):
    """NaN, +Inf and -Inf gradient elements in a full chunk, in the partial chunk and in the scalar
    kernel's second workgroup: p and the buffer are NaN where the gradient is, at damp1 (0 * inf)
    the buffer and at lr_0 (-0 * inf) the parameter at the Inf elements as well."""
    def make(kind):
        case = _SpaceCase(kind, cls, point, special=True)
        want = case.reference()
        nan = np.array(case.special_at)
        inf = np.concatenate([[64, 65], nan[1:] + 1, nan[1:] + 2])  # _adam_space.special_grads
        p = case.param(want)
        assert np.isnan(p[nan]).all() and np.isnan(want["buf"][nan]).all()
        if point == "lr_0":
            assert np.isnan(p[inf]).all() and np.isinf(want["buf"][inf]).all()
        if point == "damp1":
            assert np.isnan(want["buf"][inf]).all()
        return case

    _each_kind(gpu, make)
