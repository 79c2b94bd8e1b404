"""Per-parameter update and weight norms at the kernel level: the stats instances of the fused Adam
update (zs_adamset_run_stats), their slot layout (zs_adamset_update_norm_slots) and the finishing
kernel (zs_update_norms), with zs_sqnorm_reduce_params between them.

Every expected value comes from numpy: the master is snapshot before and after a run (the split
master joined as (hi << 16) + sext(lo)), d = after - before is one float32 subtraction and the sums
of d^2 and of after^2 are float64.  The trajectory is compared with the matching existing run
(zs_adamset_run / _run_clipped / _run_guarded) bit for bit, not with a restatement.

The bound is the project's own (DESIGN.md §4 "Error bound"): fp32 arithmetic covers one lane's K
terms of one chunk (K = 16 split master, 8 otherwise, 1 in the scalar table), all above is double
and the result is rounded to fp32 once: (K + 2) * 2^-24 relative on a segment's sum, half of that
plus 2^-24 on its norm.  The inputs keep every d^2 at or above 2^-126 (checked on the host), so no
term leaves the normal range of fp32.

The slot rule (include/zero_amd.h): 4 slots per chunk of a segment's vector part (C = 4,096
elements for the split master, 2,048 otherwise), then 4 per 256-element chunk of its scalar part;
two planes of that many doubles, the update's first.
"""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_gradnorm import SLACK, _layout, _tune
from test_update_norms_host import slot_counts

pytestmark = pytest.mark.gpu

KINDS = ("f32", "master", "split", "split_f32g")  # (gradient dtype, master storage) pairs
CHUNK = {"f32": 2048, "master": 2048, "split": 4096, "split_f32g": 4096}
TERMS = {"f32": 8, "master": 8, "split": 16, "split_f32g": 16}
MODES = ("unclipped", "clipped", "guarded")
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
SENTINEL = -7.0
NO_GRAD, SHIFTED = (7,), (5,)


def _lengths(C):
    return [0, 1, 3, 4, 255, 1024, C - 4, C, C + 4, 3 * C + 1028]


def _g32(kind):
    return kind in ("f32", "split_f32g")


class _Case:
    """Host inputs over ``segs`` = [(offset, n, has_grad)] that keep every d away from zero: the
    master lies in 0.01 .. 0.05 by magnitude, exp_avg and every gradient carry the master's sign
    and exp_avg_sq is at least 1e-4, so Adam's step (at most about lr = 1e-3 here) and the
    decoupled weight decay (at least 1e-6) push every element towards zero together, by far more
    than an ulp, and no master changes sign within the steps taken."""

    CFG = dict(lr=1e-3, wd=0.1)

    def __init__(self, kind, segs, seed, steps=2):
        self.kind, self.segs = kind, segs
        rng = np.random.default_rng(seed)
        self.N = N = max([o + n for o, n, _ in segs]) + SLACK
        sign = rng.choice([-1.0, 1.0], N)
        master = (rng.uniform(0.01, 0.05, N) * sign).astype(np.float32)
        self.init = {"m": (np.abs(rng.standard_normal(N)) * 1e-2 * sign).astype(np.float32),
                     "v": (rng.standard_normal(N) ** 2 * 1e-4 + 1e-4).astype(np.float32)}
        if kind.startswith("split"):
            self.init["hi"], self.init["lo"] = c_oracle.split_master(master)
        else:
            self.init["p"] = master
            if kind == "master":
                self.init["pb"] = zo.f32_to_bf16_bits(master)
        self.grads = []
        for _ in range(steps):
            g = (np.abs(rng.standard_normal(N)) * 1e-2 * sign).astype(np.float32)
            self.grads.append(g if _g32(kind) else zo.f32_to_bf16_bits(g))

    def master(self, arrays):
        if self.kind.startswith("split"):
            return c_oracle.join_master(arrays["hi"].view(np.uint16), arrays["lo"].view(np.uint16))
        return arrays["p"]

    def make_set(self, gpu, order=None):
        """(device tensors, gradient buffer, AdamSet); ``order``: the rows in another order."""
        import torch

        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import AdamSet

        kind = self.kind
        ints = lambda a: a.view(np.int16) if a.dtype == np.uint16 else a  # noqa: E731
        T = {k: torch.from_numpy(ints(v).copy()).to(gpu) for k, v in self.init.items()}
        G = torch.zeros(self.N, dtype=torch.float32 if _g32(kind) else torch.int16, device=gpu)
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in self.segs:
            assert 0 <= o and o + n <= self.N - SLACK
            g = G.data_ptr() + o * G.element_size() if has_g else 0
            if kind.startswith("split"):
                row = [g, at("hi", o), at("lo", o), at("hi", o)]
            else:
                row = [g, at("p", o), at("p", o), at("pb", o)]
            rows.append(row + [at("m", o), at("v", o), 0, 0, n])
        rows = np.array(rows, dtype=np.uint64)
        if order is not None:
            rows = rows[np.asarray(order)]
        aset = AdamSet(rows, ZS_F32 if _g32(kind) else ZS_BF16,
                       ZS_BF16_SPLIT if kind.startswith("split") else ZS_BF16,
                       wide_grads=kind == "split_f32g")
        return T, G, aset


class _Run:
    """One set on the GPU, stepped through ``run_stats`` (``stats``) or the matching existing run."""

    def __init__(self, gpu, case, stats, mode, coef=np.float32(0.37), order=None):
        import torch

        self.case, self.stats, self.mode, self.gpu = case, stats, mode, gpu
        self.T, self.G, self.aset = case.make_set(gpu, order)
        self.cbuf = None if mode == "unclipped" else \
            torch.from_numpy(np.array([coef], np.float32)).to(gpu)
        self.st = torch.cuda.current_stream()
        self.off = self.aset.update_norm_offsets
        self.n = int(self.off[-1])
        self.partials = torch.full((2 * self.n + 8,), SENTINEL, dtype=torch.float64, device=gpu)
        self.t = 0

    def step(self):
        import torch

        from zero_amd.kernels import adam_hparams

        case, g = self.case, self.case.grads[self.t]
        self.t += 1
        self.G.copy_(torch.from_numpy(g if g.dtype == np.float32 else g.view(np.int16)))
        hp = adam_hparams(case.CFG["lr"], 0.9, 0.999, 1e-8, case.CFG["wd"], self.t + 2, decoupled=True,
                          grad_div=3.0 if self.mode != "unclipped" else 1.0)
        guard = self.mode == "guarded"
        if self.stats:
            self.partials.fill_(SENTINEL)
            self.aset.run_stats(hp, self.partials, self.st, coef=self.cbuf, guard=guard)
        elif self.cbuf is None:
            self.aset.run(hp, self.st)
        elif guard:
            self.aset.run_guarded(hp, self.cbuf, self.st)
        else:
            self.aset.run_clipped(hp, self.cbuf, self.st)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.T.items()}

    def planes(self):
        """(update plane, weight plane) as float64; nothing was written behind them."""
        part = self.partials.cpu().numpy()
        assert (part[2 * self.n:] == SENTINEL).all(), "a partial was written past the set's slots"
        return part[:self.n].copy(), part[self.n:2 * self.n].copy()

    def reduce(self, coef=None, touched=None, weight0=None):
        """Per-segment sums through zs_sqnorm_reduce_params (one parameter per segment) and the
        norms through zs_update_norms: (sums of d^2, sums of p1^2, update norms, weight norms)."""
        import torch

        from zero_amd.kernels import sqnorm_reduce_params, update_norms

        ns, cnt = len(self.off) - 1, np.diff(self.off)
        live = np.flatnonzero(cnt > 0)
        dev = lambda a: torch.from_numpy(np.asarray(a, np.int64).copy()).to(self.gpu)  # noqa: E731
        row_ptr = dev(np.concatenate([[0], np.cumsum(cnt > 0)]))
        sums3 = torch.zeros(3 * ns, device=self.gpu)
        for plane in (0, 1):
            sqnorm_reduce_params(self.partials, row_ptr, dev(plane * self.n + self.off[:-1][live]),
                                 dev(cnt[live]), ns, sums3[plane * ns:], self.st)
        sums3[2 * ns:] = torch.from_numpy(np.asarray(
            (cnt > 0) if touched is None else touched, np.float32)).to(self.gpu)
        un = torch.full((ns,), 5.0, device=self.gpu)
        wn = torch.from_numpy(np.full(ns, 9.0, np.float32) if weight0 is None else weight0).to(self.gpu)
        cbuf = None if coef is None else torch.from_numpy(np.array([coef], np.float32)).to(self.gpu)
        update_norms(sums3, ns, cbuf, un, wn, self.st)
        torch.cuda.synchronize()
        s = sums3.cpu().numpy()
        return s[:ns].copy(), s[ns:2 * ns].copy(), un.cpu().numpy(), wn.cpu().numpy()


def _want(p0, p1, segs):
    """Per segment, in float64: (sum of d^2, sum of p1^2), d one float32 subtraction."""
    d = (p1 - p0).astype(np.float32)
    assert d.dtype == np.float32
    wd, ww = [], []
    for o, n, _ in segs:
        dd = d[o:o + n].astype(np.float64) ** 2
        assert (dd >= 2.0 ** -126).all(), "an input element's d^2 is below the normal range"
        wd.append(dd.sum())
        ww.append((p1[o:o + n].astype(np.float64) ** 2).sum())
    return np.array(wd), np.array(ww)


def _bound(kind, segs, shifted):
    """(K + 2) * 2^-24 per segment: K of the vector table where the segment has a vector part."""
    return np.array([((TERMS[kind] if (k not in shifted and n >= 4) else 1) + 2) * 2.0 ** -24
                     for k, (_, n, _) in enumerate(segs)])


def _check(kind, what, got, want, norms, bound):
    worst = worst_n = 0.0
    for i, (a, w) in enumerate(zip(got, want)):
        if w == 0.0:  # the zero-length segment
            assert a == 0.0 and not np.signbit(a), (what, i, a)
            continue
        rel = abs(float(a) - w) / w
        rel_n = abs(float(norms[i]) - np.sqrt(w)) / np.sqrt(w)
        worst, worst_n = max(worst, rel / bound[i]), max(worst_n, rel_n / (bound[i] / 2 + 2.0 ** -24))
        assert rel <= bound[i], (what, i, rel, bound[i])
        assert rel_n <= bound[i] / 2 + 2.0 ** -24, (what, i, rel_n)
    print(f"{kind} {what}: worst sum error {worst:.3f} of its bound, worst norm error {worst_n:.3f}")


_cases = {}


def _case(kind):
    """One mixed table per kind, shared by the tests (the inputs are never written)."""
    if kind not in _cases:
        segs = _layout(_lengths(CHUNK[kind]), no_grad=NO_GRAD, shifted=SHIFTED)
        _cases[kind] = _Case(kind, segs, seed=70 + KINDS.index(kind))
    return _cases[kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_trajectory_sums_and_slots(gpu, kind, mode):
    """Two steps over the mixed table: every array equals the matching existing run's bit for bit;
    the slot offsets follow the rule, every slot of both planes is written and nothing behind
    them; each segment's sums and norms hold their bound against float64."""
    case = _case(kind)
    segs = case.segs
    a, b = _Run(gpu, case, True, mode), _Run(gpu, case, False, mode)
    want_off = np.concatenate([[0], np.cumsum(slot_counts(CHUNK[kind], segs, SHIFTED))])
    assert np.array_equal(a.off, want_off), (a.off, want_off)
    assert a.off[1] == a.off[0]  # the zero-length segment has no slots
    bound = _bound(kind, segs, SHIFTED)
    before = {k: v.copy() for k, v in case.init.items()}
    for step in (1, 2):
        got, ref = a.step(), b.step()
        for name in ref:
            assert np.array_equal(got[name].view(np.uint8), ref[name].view(np.uint8)), (step, name)
        pd, pw = a.planes()
        assert (pd != SENTINEL).all() and (pw != SENTINEL).all(), "a slot was not written"
        assert (pd >= 0).all() and (pw >= 0).all()
        wd, ww = _want(case.master(before), case.master(got), segs)
        sd, sw, un, wn = a.reduce()
        _check(kind, f"{mode} step {step} update", sd, wd, un, bound)
        _check(kind, f"{mode} step {step} weight", sw, ww, wn, bound)
        # the finishing kernel is the restated formula on the reduced sums, bit for bit
        with np.errstate(all="ignore"):
            live = np.diff(a.off) > 0
            ru = np.where(live, np.sqrt(sd.astype(np.float64)).astype(np.float32), np.float32(0))
            rw = np.where(live, np.sqrt(sw.astype(np.float64)).astype(np.float32), np.float32(9))
        assert np.array_equal(un.view(np.uint32), ru.view(np.uint32))
        assert np.array_equal(wn.view(np.uint32), rw.view(np.uint32))
        before = got


@pytest.mark.parametrize("kind", KINDS)
def test_bits_do_not_depend_on_run_grid_body_or_order(gpu, kind):
    """A table with more chunks than one workgroup per CU has workgroups: the partials have the
    same bits from run to run, under a grid cap that makes every workgroup stride, through the
    predicated body alone (adam_loads_first = 0) and with the rows in another order (each
    segment's slots then stand elsewhere and hold the same bits)."""
    import torch

    C = CHUNK[kind]
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    segs = _layout([1, 255, C + 4, (cus + 40) * C + 1028 + 2, 5000], shifted=(4,))
    case = _Case(kind, segs, seed=90 + KINDS.index(kind), steps=1)

    def planes(order=None):
        r = _Run(gpu, case, True, "clipped", order=order)
        r.step()
        pd, pw = r.planes()
        return r.off, pd.view(np.uint64), pw.view(np.uint64)

    off, pd, pw = planes()
    _, pd2, pw2 = planes()
    assert np.array_equal(pd, pd2) and np.array_equal(pw, pw2), "run to run"
    for key, value, back in ((b"adam_wg_per_cu", 1, 0), (b"adam_loads_first", 0, 1)):
        _tune(key, value)
        try:
            _, pd2, pw2 = planes()
        finally:
            _tune(key, back)
        assert np.array_equal(pd, pd2) and np.array_equal(pw, pw2), key
    order = [3, 0, 4, 2, 1]
    off2, pd2, pw2 = planes(order)
    for k2, k in enumerate(order):
        assert off2[k2 + 1] - off2[k2] == off[k + 1] - off[k]
        for x, y in ((pd, pd2), (pw, pw2)):
            assert np.array_equal(x[off[k]:off[k + 1]], y[off2[k2]:off2[k2 + 1]]), ("permuted", k)


@pytest.mark.parametrize("kind", KINDS)
def test_a_skipped_step_measures_nothing(gpu, kind):
    """A guarded run with a NaN coefficient writes no partial and changes no state; zs_update_norms
    then gives +0.0 update norms and leaves a pre-filled weight vector as it was -- as it does, with
    a finite coefficient, for the parameters whose touched mark is 0."""
    case = _case(kind)
    r = _Run(gpu, case, True, "guarded", coef=QNAN)
    got = r.step()
    for name, ref in case.init.items():
        assert np.array_equal(got[name].view(np.uint8), ref.view(np.uint8)), name
    part = r.partials.cpu().numpy()
    assert (part == SENTINEL).all(), "a skipped step wrote a partial"
    ns = len(case.segs)
    w0 = np.arange(1, ns + 1, dtype=np.float32)
    _, _, un, wn = r.reduce(coef=QNAN, weight0=w0)
    assert (un.view(np.uint32) == 0).all()  # +0.0
    assert np.array_equal(wn, w0)
    # a taken step; parameters 2 and 9 are marked untouched
    r2 = _Run(gpu, case, True, "guarded")
    r2.step()
    touched = (np.diff(r2.off) > 0).astype(np.float32)
    touched[[2, 9]] = 0.0
    _, sw, un, wn = r2.reduce(coef=np.float32(0.37), touched=touched, weight0=w0)
    assert un[2].view(np.uint32) == 0 and un[9].view(np.uint32) == 0
    assert wn[2] == w0[2] and wn[9] == w0[9]
    for i in (3, 8):
        assert un[i] > 0 and wn[i] == np.float32(np.sqrt(np.float64(sw[i])))


def test_refusals_that_need_segments(gpu):
    """A set with the vmax column, a set with bf16 state: ZS_ERR_INVALID, nothing launched; a set
    with slots and NULL partials likewise."""
    import torch

    from zero_amd import _lib
    from zero_amd.kernels import AdamSet, adam_hparams

    case = _Case("f32", [(0, 2048 + 4, True)], seed=3, steps=1)
    hp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    st = torch.cuda.current_stream()
    T, G, aset = case.make_set(gpu)
    buf = torch.zeros(2 * int(aset.update_norm_offsets[-1]), dtype=torch.float64, device=gpu)
    with pytest.raises(_lib.ZeroAmdError, match="zs_adamset_run_stats: .*guard") as e:
        aset.run_stats(hp, buf, st, guard=True)
    assert e.value.code == _lib.ZS_ERR_INVALID
    with pytest.raises(_lib.ZeroAmdError, match="zs_adamset_run_stats: partials is NULL"):
        aset.run_stats(hp, 0, st)
    x = torch.zeros(case.N, device=gpu)
    rows = np.array([[G.data_ptr(), T["p"].data_ptr(), T["p"].data_ptr(), 0, T["m"].data_ptr(),
                      T["v"].data_ptr(), x.data_ptr(), 0, 2052]], np.uint64)
    with pytest.raises(_lib.ZeroAmdError, match="zs_adamset_run_stats: .*vmax"):
        AdamSet(rows, _lib.ZS_F32, _lib.ZS_BF16).run_stats(hp, buf, st)
    rows[0, 6], rows[0, 7] = 0, x.data_ptr()
    with pytest.raises(_lib.ZeroAmdError, match="zs_adamset_run_stats: .*carry"):
        AdamSet(rows, _lib.ZS_F32, _lib.ZS_BF16).run_stats(hp, buf, st)
    torch.cuda.synchronize()
    for name, ref in case.init.items():
        assert np.array_equal(T[name].cpu().numpy().view(np.uint8), ref.view(np.uint8)), name
