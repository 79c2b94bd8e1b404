"""The fused Schedule-Free AdamW kernels (SfAdamRule through the update kernel pair, the two swap
kernels) over the hyperparameter and magnitude space of tests/_sfadam_space.py, bit for bit against
tests/_sfadam_oracle.py (which tests/test_sfadam_oracle.py pins to the class itself over the same
space).

One step, or one swap, from a planted y, z, v (and carry), per grid point, magnitude class and kind,
over one table that reaches every kernel path (C = 4,096 elements for a split master, 2,048
otherwise):
  (0, 2C+4, gradient)   full chunks (the loads-first body) and a partial chunk (the predicated one)
  one element off alignment, n = 261, gradient: the scalar kernel, two workgroups
  aligned, n = 7, no gradient: the vector kernel's first 4 and a 3-element scalar tail, g = 0
A segment without a gradient is a contract of the kernels alone: g = 0, so v still decays and the
weight decay and the lerp still apply; the oracle is fed zeros.  The class skips such a parameter
and the wrappers never pass one.

Every array the kernels may write is compared whole (gaps between the segments and 4,096 elements
of slack behind the last one included), the update with ``adam_loads_first`` at 0 and at 1 (the
swap kernels do not read that switch).  A NaN need only be a NaN, and the residual of a NaN split
master reads 0.  Under 15k elements per case but one.

Kinds: ``split`` (bf16 gradient, split master), ``bf16`` (bf16 gradient, fp32 master and its bf16
copy), ``f32`` (fp32 gradient and parameter) and ``f32split`` (fp32 gradient over the split master,
ZeRO-3 after an fp32-accumulated step).  The library has no carry instance of ``f32split`` and
refuses one when the set is made: test_carry runs the other three, and
test_carry_over_f32split_is_refused holds the refusal.
"""
import numpy as np
import pytest
import torch

import _sfadam_oracle as so
import _sfadam_space as sp
from test_gpu_lion_kernel import _layout, _tune
from test_gpu_sfadam_kernel import CHUNK, SLACK

pytestmark = pytest.mark.gpu

KINDS = ("split", "bf16", "f32", "f32split")
CLIP_COEF = np.float32(0.3)  # 0x3E99999A: no power of two, so g * coef rounds


def _table(C):
    return _layout([(2 * C + 4, True, 0), (261, True, 1), (7, False, 0)])


class _SpaceCase:
    """``ops`` ("step", "eval", "train") in order from a planted state; the step with the
    hyperparameters of one grid point, the swaps with ``beta1``'s two weights."""

    def __init__(self, kind, cls, ops=("step",), *, point="default", beta1=0.9, carry=None,
                 clip=False, special=False, special_y=False, spec=None, seed=5):
        self.kind, self.ops, self.clip, self.beta1 = kind, tuple(ops), clip, beta1
        self.carry = carry is not None
        self.hp = sp.hp_of(point)
        if carry is not None:
            self.hp.update(grad_div=carry[0], carry_mul=carry[1])
        elif clip:
            self.hp.update(grad_div=3.0)
        self.split = kind in ("split", "f32split")
        self.wide_g = kind in ("f32", "f32split")
        C = CHUNK[kind]
        self.segs = _table(C) if spec is None else _layout(spec(C))
        self.N = N = max(o + n for o, n, _ in self.segs) + SLACK
        assert spec is not None or N - SLACK < 15000
        s = sp.planted(cls, N, seed)
        # specials in a full chunk, in the partial chunk and in the scalar kernel's second workgroup
        self.special_at = (3, 2 * C, self.segs[1][0] + 257)
        g = sp.special_grads(s, more=self.special_at[1:]) if special else s["g"]
        self.g = g.copy() if self.wide_g else so.f32_to_bf16_bits(g)
        if special_y:  # +Inf, -Inf and NaN parameters at the same three places
            s = dict(s, y=sp.special_params(s, more=self.special_at[1:]))
        self.state0 = {"z": s["z"], "v": s["v"]}
        if self.carry:
            self.state0["carry"] = s["carry"]
        if self.split:
            self.state0["hi"], self.state0["lo"] = sp.split_master(s["y"])
        else:
            self.state0["p"] = s["y"]
            if kind == "bf16":
                self.state0["pb"] = np.zeros(N, np.uint16)

    @staticmethod
    def _canon(out):
        return {k: sp.canon(np.ascontiguousarray(a), out["hi"] if k == "lo" else None).view(
            np.float32 if a.itemsize == 4 else np.uint16) for k, a in out.items()}

    def param(self, out):
        """The fp32 y (or x) of one stage of ``reference`` / ``run_gpu``."""
        return sp.join_master(out["hi"], out["lo"]) if self.split else out["p"]

    # ---- the numpy restatement, segment by segment on slices of the arena ----
    def reference(self):
        """The arrays after every op, canonicalised."""
        out = {k: a.copy() for k, a in self.state0.items()}
        hp = so.SfHP(**self.hp)
        coef = CLIP_COEF if self.clip else None
        stages = []
        for op in self.ops:
            for o, n, has_g in self.segs:
                sl = slice(o, o + n)
                y = sp.join_master(out["hi"][sl], out["lo"][sl]) if self.split else out["p"][sl]
                shown = None  # what the bf16 copy shows, where it is not the master rounded
                if op == "step":
                    g = self.g[sl].copy()
                    if not has_g:
                        g[:] = 0
                    res = so.sfadam_elem(g, y, out["z"][sl], out["v"][sl], hp, coef=coef,
                                         carry=out["carry"][sl] if self.carry else None)
                    y, out["z"][sl], out["v"][sl] = res[:3]
                    if self.carry:
                        out["carry"][sl] = res[3]
                elif self.kind == "bf16":  # the copy alone moves: eval shows x, train the master
                    shown = so.swap(y, out["z"][sl], self.beta1, True) if op == "eval" else y
                else:
                    y = so.swap(y, out["z"][sl], self.beta1, op == "eval")
                if self.split:
                    out["hi"][sl], out["lo"][sl] = sp.split_master(y)
                else:
                    out["p"][sl] = y
                    if self.kind == "bf16":
                        out["pb"][sl] = so.f32_to_bf16_bits(y if shown is None else shown)
            stages.append(self._canon(out))
        return stages

    # ---- the kernels ----
    def run_gpu(self, gpu, loads_first=1, wg_per_cu=0):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import SfAdamSet, sfadam_hparams

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
            rows.append(row + [at("z", o), at("v", o), 0, at("carry", o), n])
        sset = SfAdamSet(np.array(rows, dtype=np.uint64), ZS_F32 if self.wide_g else ZS_BF16,
                         ZS_BF16_SPLIT if self.split else ZS_BF16, wide_grads=self.wide_g)
        hp = sfadam_hparams(**self.hp)
        coef = torch.from_numpy(np.array([CLIP_COEF])).to(gpu) if self.clip else None
        st = torch.cuda.current_stream()
        stages = []
        _tune(b"adam_loads_first", loads_first)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            for op in self.ops:
                if op == "step":
                    sset.run(hp, st, coef=coef)
                elif op == "eval":
                    sset.swap(1 - 1 / self.beta1, True, st)
                else:
                    sset.swap(1 - self.beta1, False, st)
                torch.cuda.synchronize()
                out = {k: v.cpu().numpy() for k, v in T.items()}
                stages.append(self._canon({k: a.view(np.uint16) if a.itemsize == 2 else a
                                           for k, a in out.items()}))
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        return stages


def _bits(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint16)


def _check(gpu, case, wg_per_cu=0, loads_first=(0, 1)):
    want = case.reference()
    got = []
    for lf in loads_first:
        got = case.run_gpu(gpu, lf, wg_per_cu)
        assert len(got) == len(want) == len(case.ops)
        for op, w, g in zip(case.ops, want, got):
            assert set(g) == set(w)
            for name, ref in w.items():
                bad = np.flatnonzero(_bits(g[name]) != _bits(ref))
                assert bad.size == 0, (f"after {op}: {name}, adam_loads_first={lf}: {bad.size} "
                                       f"elements differ from the oracle, first at {bad[:8]}")
    return want, got


def _each_kind(gpu, make, kinds=KINDS, after=None, **kw):
    """``_check`` on ``make(kind)`` for every kind, then ``after(case, want, got)``.  Every kind
    runs whatever the ones before it gave, and the test fails with all their differences.  (The
    kinds share one test item: one kind's part of the body takes a few milliseconds, the suite's
    collection of garbage after every item many times that.)"""
    failed = []
    for kind in kinds:
        case = make(kind)
        try:
            want, got = _check(gpu, case, **kw)
            if after is not None:
                after(case, want, got)
        except AssertionError as e:
            failed.append(f"{kind}: {e}")
    assert not failed, "\n".join(failed)


def _inside(case):
    inside = np.zeros(case.N, bool)
    for o, n, _ in case.segs:
        inside[o:o + n] = True
    return inside


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", list(sp.GRID))
def test_grid(gpu, point, cls):
    """Every grid point, one step from the planted state, every kind."""
    def moved(case, want, got):  # (and the reference is not the planted state)
        changed = _bits(want[0]["v"]) != sp.canon(case.state0["v"])
        assert changed[_inside(case)].mean() > 0.5 and not changed[~_inside(case)].any()

    _each_kind(gpu, lambda kind: _SpaceCase(kind, cls, point=point), after=moved)


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("div,mul", [(3.0, 2.0), (2.0, 1.0)])
@pytest.mark.parametrize("point", ["default", "all", "c_1"])
def test_carry(gpu, point, div, mul, cls):
    """The ZeRO-1 carry with a true division (3) and a reciprocal multiply (2): the CARRY
    instances of the three kinds that have one, the carry array compared as well."""
    def moved(case, want, got):
        assert (_bits(want[0]["carry"]) != sp.canon(case.state0["carry"])).mean() > 0.5

    _each_kind(gpu, lambda kind: _SpaceCase(kind, cls, point=point, carry=(div, mul)), KINDS[:3],
               moved)


def test_carry_over_f32split_is_refused(gpu):
    """``f32split`` has no CARRY instance: the set is refused when it is made, whatever the point,
    class and divisor, so test_carry cannot run it."""
    from zero_amd._lib import ZS_ERR_INVALID, ZeroAmdError

    assert KINDS[3:] == ("f32split",)
    with pytest.raises(ZeroAmdError, match="takes no carry") as e:
        _SpaceCase("f32split", "normal", carry=(3.0, 2.0)).run_gpu(gpu)
    assert e.value.code == ZS_ERR_INVALID


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", ["all", "default"])
def test_clipped(gpu, point, cls):
    """The coefficient 0.3 (no power of two) read from device memory, with grad_div = 3: the CLIP
    instances of all four kinds."""
    def differs(case, want, got):  # (the coefficient reached the reference)
        plain = _SpaceCase(case.kind, cls, point=point).reference()
        assert (_bits(want[0]["v"]) != _bits(plain[0]["v"]))[_inside(case)].mean() > 0.5

    _each_kind(gpu, lambda kind: _SpaceCase(kind, cls, point=point, clip=True), after=differs)


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", ["default", "eps_0", "lr_0", "wd"])
def test_nan_inf(gpu, point, cls):
    """NaN, +Inf and -Inf gradient elements in a full chunk, in the partial chunk and in the scalar
    kernel's second workgroup.  A NaN gradient makes y, z and v NaN.  An infinite one makes v
    +Inf, so n = Inf / (sqrt(Inf) + eps) = Inf / Inf is NaN, and y and z with it.  At lr_0 both
    ``a`` and ``-lr_t`` are -0.0: -0 * NaN is NaN, so the special elements are NaN all the same,
    while z = fma(-0, n, z) keeps its value at every finite gradient and y there is the lerp
    alone (plus a zero)."""
    def make(kind):
        case = _SpaceCase(kind, cls, point=point, special=True)
        want = case.reference()[0]
        nan = np.array(case.special_at)
        inf = np.concatenate([[64, 65], nan[1:] + 1, nan[1:] + 2])  # _adam_space.special_grads
        y = case.param(want)
        for a in (y, want["z"], want["v"]):
            assert np.isnan(a[nan]).all()
        assert (want["v"][inf] == np.inf).all()
        assert np.isnan(y[inf]).all() and np.isnan(want["z"][inf]).all()
        if kind == "bf16":
            assert (want["pb"][np.concatenate([nan, inf])] & 0x7FFF > 0x7F80).all()
        if point == "lr_0":
            fin = np.ones(case.N, bool)
            fin[np.concatenate([nan, inf])] = False
            assert np.array_equal(want["z"][fin], case.state0["z"][fin])  # (as numbers)
        return case

    _each_kind(gpu, make)


@pytest.mark.parametrize("cls", sp.CLASSES)
@pytest.mark.parametrize("point", ["default", "c_0.5", "wd"])
def test_infinite_parameter(gpu, point, cls):
    """+Inf, -Inf and NaN in y, in a full chunk, in the partial chunk and in the scalar kernel's
    second workgroup.  Without weight decay y enters through the lerp alone, so z and v come out
    as from a finite y (an fma(0, y, n) run all the same would make z NaN there); with it
    0.1 * Inf reaches n and z.  The high form of the lerp (c = 0.5) keeps an infinite y, the low
    one makes it NaN (Inf - Inf)."""
    def make(kind):
        case = _SpaceCase(kind, cls, point=point, special_y=True)
        want = case.reference()[0]
        far = np.array(case.special_at[1:])
        inf = np.concatenate([[5, 66], far, far + 1])  # _sfadam_space.special_params
        at = np.concatenate([inf, [67], far + 2])
        y0, y = case.param(case._canon(case.state0)), case.param(want)
        assert np.isinf(y0[inf]).all() and np.isnan(y0[at[len(inf):]]).all()
        if point == "wd":
            assert not np.isfinite(want["z"][at]).any()
        else:
            plain = _SpaceCase(kind, cls, point=point).reference()[0]
            assert np.array_equal(_bits(want["z"]), _bits(plain["z"]))
            assert np.isfinite(want["z"][at]).all()
            assert (np.isinf(y[inf]) if point == "c_0.5" else np.isnan(y[inf])).all()
        return case

    _each_kind(gpu, make)


def _forms(beta1):
    """(eval, train): whether the reference's swap takes ATen's high form, fma(w - 1, z - p, z),
    decided by comparing it with both forms written out."""
    s = sp.planted("normal")
    p, z = s["y"], s["z"]
    out = []
    for to_eval, w in ((True, 1 - 1 / beta1), (False, 1 - beta1)):
        w = np.float32(w)
        low = so.fma32(w, z - p, p)
        high = so.fma32(np.float32(w - np.float32(1)), z - p, z)
        assert (sp.canon(low) != sp.canon(high)).any()  # the two can be told apart (-999: 4 do)
        ref = sp.canon(so.swap(p, z, beta1, to_eval))
        is_high = np.array_equal(ref, sp.canon(high))
        assert is_high or np.array_equal(ref, sp.canon(low))
        out.append(is_high)
    return tuple(out)


def test_swap_points_take_both_forms():
    """The reference alone: train's weight 1 - beta1 takes the high form for beta1 <= 0.5, eval's
    1 - 1/beta1 for beta1 <= 2/3, both boundaries are points themselves, and every combination
    that exists is among the points."""
    forms = {b: _forms(b) for b in sp.SWAP_BETA1}
    for b, f in forms.items():
        assert f == (b <= 2 / 3, b <= 0.5), (b, f)
    assert forms[0.5] == (True, True) and forms[2 / 3] == (True, False)
    assert np.float32(1 - 1 / (2 / 3)) == np.float32(-0.5)  # the boundaries themselves
    assert set(forms.values()) == {(False, False), (True, False), (True, True)}


@pytest.mark.parametrize("cls", sp.SWAP_CLASSES)
@pytest.mark.parametrize("beta1", sp.SWAP_BETA1, ids=lambda b: f"b1_{b:.4g}")
def test_swap_space(gpu, beta1, cls):
    """eval() from the planted (p, z), then train() from its result, every array compared after
    each call.  z and v keep their bytes; beside a bf16 copy the fp32 master keeps its bytes both
    ways and train's copy is the master rounded again."""
    def kept(case, want, got):
        for stage in got:
            for name in ("z", "v") + (("p",) if case.kind == "bf16" else ()):
                assert np.array_equal(_bits(stage[name]), sp.canon(case.state0[name])), name
        if case.kind == "bf16":
            back = sp.canon(so.f32_to_bf16_bits(case.state0["p"]))
            assert np.array_equal(_bits(got[1]["pb"])[_inside(case)], back[_inside(case)])
        else:  # the swap moved the parameter, and train did not simply undo the bytes' change
            y0 = sp.canon(np.ascontiguousarray(case.param(case._canon(case.state0))))
            x = sp.canon(np.ascontiguousarray(case.param(want[0])))
            assert (x != y0)[_inside(case)].mean() > 0.5

    _each_kind(gpu, lambda kind: _SpaceCase(kind, cls, ("eval", "train"), beta1=beta1), KINDS[:3],
               kept, loads_first=(1,))


@pytest.mark.parametrize("kind", ["split", "f32"])
def test_swap_more_chunks_than_workgroups(gpu, kind):
    """One workgroup per CU over 301 vector chunks and 301 + 2 scalar chunks: every vector and
    every scalar workgroup walks several chunks, past an empty segment, and the scalar scan crosses
    into the next segment after it has wrapped.  One update step, then eval, then train, compared
    after each.  The one large case: about 1.3 M elements."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert cus < 300

    def spec(C):
        return [(300 * C + 4, True, 0), (0, True, 0), (300 * 256 + 3, True, 1), (261, True, 1)]

    case = _SpaceCase(kind, "normal", ("step", "eval", "train"), spec=spec)
    assert [n for _, n, _ in case.segs] == [300 * CHUNK[kind] + 4, 0, 76803, 261]
    assert all(o % 4 == 1 for o, _, _ in case.segs[2:])
    _check(gpu, case, wg_per_cu=1, loads_first=(1,))
