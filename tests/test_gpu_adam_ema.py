"""The EMA instances of the fused Adam update (zs_adamset_run_ema) against tests/_ema_oracle.py, bit
for bit (a NaN need only be a NaN).

Kinds: fp32 parameters, the fp32 master with a bf16 parameter out (chunk C = 2,048 elements), and
the split master with bf16 and with fp32 gradients (C = 4,096).  Every case runs 3 steps over
tests/test_gpu_adam_chunks.py's mixed table -- full chunks, a segment shorter than a chunk, one
without a gradient, one unaligned (the scalar kernel), a partial last chunk -- with
``adam_loads_first`` at 0 and at 1, and compares every array the kernel writes whole, gaps between
segments and the slack behind the last one included, against the oracle and between the two
settings.  The master carries that file's tie / denormal / overflow-edge plants, the gradients NaN
and +-inf; the state arrays start from random values everywhere.
"""
import numpy as np
import pytest
import torch

import _ema_oracle as eo
from oracle import c_oracle
from oracle import zero_oracle as zo
from test_gpu_adam_chunks import SLACK, TIES, _mixed_table, _tune

pytestmark = pytest.mark.gpu

KINDS = ("f32", "master", "split", "split_f32g")
CHUNK = {"f32": 2048, "master": 2048, "split": 4096, "split_f32g": 4096}
STEPS = 3
# (decay, Adam configuration): 0.999 the low form of the lerp, 0.5 the boundary (high form), 0.3,
# and the two ends; AdamW, coupled weight decay, maximize
COMBOS = [(0.999, dict(weight_decay=1e-2, decoupled=True)), (0.5, dict(weight_decay=1e-2)),
          (0.3, dict(maximize=True)), (0.0, dict()), (1.0, dict(weight_decay=1e-2, maximize=True))]
COMBO_IDS = ["d0.999-adamw", "d0.5-wd", "d0.3-maximize", "d0", "d1-wd-maximize"]
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _g32(kind):
    return kind in ("f32", "split_f32g")


class _Case:
    """Host inputs of one case over ``segs`` = [(offset, n, has_grad)]."""

    def __init__(self, kind, segs, seed):
        self.kind, self.segs = kind, segs
        rng = np.random.default_rng(seed)
        self.N = N = max(o + n for o, n, _ in segs) + SLACK
        master = (rng.standard_normal(N) * 0.02).astype(np.float32)
        u = master.view(np.uint32)
        for o, n, _ in segs:  # ties at the head of every segment and of its second chunk
            for at in (o, o + CHUNK[kind]):
                k = max(0, min(len(TIES), o + n - at))
                u[at:at + k] = TIES[:k]
        with np.errstate(over="ignore"):  # (next to FLT_MAX the EMA may start at infinity)
            ema = (master * (1 + rng.standard_normal(N) * 1e-3)).astype(np.float32)
        self.init = {"m": (rng.standard_normal(N) * 1e-2).astype(np.float32),
                     "v": (rng.standard_normal(N) ** 2 * 1e-4).astype(np.float32), "ema": ema}
        if kind.startswith("split"):
            self.init["hi"], self.init["lo"] = c_oracle.split_master(master)
        else:
            self.init["p"] = master
            if kind == "master":
                self.init["pb"] = zo.f32_to_bf16_bits(rng.standard_normal(N).astype(np.float32))
        self.grads = []
        for _ in range(STEPS):
            g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
            for o, n, has_g in segs:
                if has_g and n >= 60:
                    g[o + 5], g[o + 17], g[o + 29], g[o + n - 1] = np.nan, np.inf, -np.inf, np.nan
            self.grads.append(g if _g32(kind) else zo.f32_to_bf16_bits(g))

    def reference(self, decay, cfg, coef=None, div=1.0, steps=STEPS):
        out = {k: v.copy() for k, v in self.init.items()}
        for t in range(1, steps + 1):
            hp = c_oracle.hparams(step=t, **cfg)  # (a divisor of 1: prep has divided)
            for o, n, has_g in self.segs:
                sl = slice(o, o + n)
                g = self.grads[t - 1][sl] if has_g else np.zeros(n, np.float32)
                g = eo.prep(g, div, coef)
                s = {k: v[sl] for k, v in out.items()}
                if self.kind == "f32":
                    eo.adam_ema_f32(s["p"], g, s["m"], s["v"], s["ema"], hp, decay)
                elif self.kind == "master":
                    eo.adam_ema_master(s["p"], s["pb"], g, s["m"], s["v"], s["ema"], hp, decay)
                else:
                    eo.adam_ema_split(s["hi"], s["lo"], g, s["m"], s["v"], s["ema"], hp, decay)
        return out

    def make_set(self, gpu, ema_col=True, carry=False):
        """(device tensors, gradient buffer, AdamSet) from the initial arrays."""
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import AdamSet

        kind = self.kind
        ints = lambda a: a.view(np.int16) if a.dtype == np.uint16 else a  # noqa: E731
        T = {k: torch.from_numpy(ints(v).copy()).to(gpu) for k, v in self.init.items()}
        if carry:
            T["carry"] = torch.zeros(self.N, device=gpu)
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
            rows.append(row + [at("m", o), at("v", o), at("ema", o) if ema_col else 0,
                               at("carry", o), n])
        aset = AdamSet(np.array(rows, dtype=np.uint64), ZS_F32 if _g32(kind) else ZS_BF16,
                       ZS_BF16_SPLIT if kind.startswith("split") else ZS_BF16,
                       wide_grads=kind == "split_f32g")
        return T, G, aset

    def run_gpu(self, gpu, decay, cfg, lf, wg_per_cu=0, coef=None, guard=False, div=1.0,
                steps=STEPS, ema_col=True):
        """``coef``: the coefficient's fp32 value, read from device memory (clipped / guarded);
        ``ema_col=False``: a set without the column, through run / run_clipped."""
        from zero_amd.kernels import adam_hparams

        T, G, aset = self.make_set(gpu, ema_col)
        cbuf = None if coef is None else torch.from_numpy(np.array([coef], np.float32)).to(gpu)
        st = torch.cuda.current_stream()
        _tune(b"adam_loads_first", lf)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            for t in range(1, steps + 1):
                g = self.grads[t - 1]
                G.copy_(torch.from_numpy(g if g.dtype == np.float32 else g.view(np.int16)))
                hp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, cfg.get("weight_decay", 0.0), t,
                                  decoupled=cfg.get("decoupled", False),
                                  maximize=cfg.get("maximize", False), grad_div=div)
                if ema_col:
                    aset.run_ema(hp, float(eo.weight(decay)), st, coef=cbuf, guard=guard)
                elif cbuf is None:
                    aset.run(hp, st)
                else:
                    aset.run_clipped(hp, cbuf, st)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        return {k: v.cpu().numpy() for k, v in T.items()}


def _compare(got, want, what):
    """Every array whole; ``lo`` is not defined where the master is a NaN (its payload is free)."""
    nan_master = None
    if "hi" in want:
        nan_master = np.isnan(c_oracle.join_master(want["hi"], want["lo"]))
    for name, ref in want.items():
        bad = eo.same_bits(got[name], ref, floats=name != "lo")
        if name == "lo":
            bad = bad[~nan_master[bad]]
        assert bad.size == 0, f"{what}, {name}: {bad.size} elements differ, first at {bad[:8]}"


def _identical(a, b, what):
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{what}: {name}"


_cases = {}


def _case(kind):
    """One mixed table per kind, shared by the tests (the inputs are never written)."""
    if kind not in _cases:
        _cases[kind] = _Case(kind, _mixed_table(CHUNK[kind]), seed=50 + KINDS.index(kind))
    return _cases[kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("decay,cfg", COMBOS, ids=COMBO_IDS)
def test_mixed_table(gpu, kind, decay, cfg):
    case = _case(kind)
    want = case.reference(decay, cfg)
    got = {lf: case.run_gpu(gpu, decay, cfg, lf) for lf in (0, 1)}
    for lf in (0, 1):
        _compare(got[lf], want, f"adam_loads_first={lf}")
    _identical(got[0], got[1], "adam_loads_first 0 against 1")
    if decay != 1.0:  # (the test would pass on a kernel that leaves the EMA alone otherwise)
        assert eo.same_bits(want["ema"], case.init["ema"]).size > case.N // 4
    if decay == 0.999:
        # one workgroup per CU: the grid is shorter than the chunk count, every workgroup strides
        chunks = sum(n // CHUNK[kind] for _, n, _ in case.segs)
        assert 2 * torch.cuda.get_device_properties(gpu).multi_processor_count <= chunks
        _compare(case.run_gpu(gpu, decay, cfg, 1, wg_per_cu=1), want, "one workgroup per CU")


@pytest.mark.parametrize("kind", KINDS)
def test_clipped_and_guarded_with_a_finite_coefficient(gpu, kind):
    """A coefficient below 1 and a divisor that is no power of two: the clipped and the guarded
    instances, the same bits."""
    case, cfg = _case(kind), dict(weight_decay=1e-2, decoupled=True)
    coef = np.float32(0.37)
    want = case.reference(0.999, cfg, coef=coef, div=3.0)
    for lf in (0, 1):
        got = case.run_gpu(gpu, 0.999, cfg, lf, coef=coef, div=3.0)
        _compare(got, want, f"clipped, adam_loads_first={lf}")
        guarded = case.run_gpu(gpu, 0.999, cfg, lf, coef=coef, guard=True, div=3.0)
        _identical(guarded, got, f"guarded against clipped, adam_loads_first={lf}")
    unclipped = case.reference(0.999, cfg, div=3.0)
    assert eo.same_bits(want["m"], unclipped["m"]).size > case.N // 2  # the coefficient acted


@pytest.mark.parametrize("kind", KINDS)
def test_nan_coefficient_changes_nothing(gpu, kind):
    case = _case(kind)
    for lf in (0, 1):
        got = case.run_gpu(gpu, 0.5, dict(weight_decay=1e-2), lf, coef=QNAN, guard=True, steps=2)
        for name, ref in case.init.items():
            assert np.array_equal(got[name].view(np.uint8), ref.view(np.uint8)), (lf, name)


@pytest.mark.parametrize("kind", ["f32", "split"])
def test_sets_without_the_column_run_as_before(gpu, kind):
    """run / run_clipped over a set without an EMA column: the C oracle's own entry points (the
    path tests/test_gpu_adam_chunks.py pins), and the EMA array, which no row points to, untouched."""
    case, cfg = _case(kind), dict(weight_decay=1e-2)
    want = {k: v.copy() for k, v in case.init.items()}
    for t in range(1, STEPS + 1):
        hp = c_oracle.hparams(step=t, **cfg)
        for o, n, has_g in case.segs:
            sl = slice(o, o + n)
            g = case.grads[t - 1][sl].copy()
            if not has_g:
                g[:] = 0
            if kind == "split":
                c_oracle.adam_bf16_split(want["hi"][sl], want["lo"][sl], g, want["m"][sl], want["v"][sl], hp)
            else:
                c_oracle.adam_f32(want["p"][sl], g, want["m"][sl], want["v"][sl], hp)
    _compare(case.run_gpu(gpu, None, cfg, 1, ema_col=False), want, "run")
    coef = np.float32(0.37)
    clipped = case.reference(0.0, cfg, coef=coef, div=2.0)
    clipped["ema"] = case.init["ema"]
    _compare(case.run_gpu(gpu, None, cfg, 1, coef=coef, div=2.0, ema_col=False), clipped, "run_clipped")


def test_refusals_that_need_segments(gpu):
    """A set with the carry and a set without the vmax column: ZS_ERR_INVALID, nothing launched."""
    from zero_amd import _lib
    from zero_amd.kernels import adam_hparams

    case = _Case("f32", [(0, 2048 + 4, True)], seed=3)
    hp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    st = torch.cuda.current_stream()
    for kw, text in ((dict(carry=True), "carry"), (dict(ema_col=False), "vmax")):
        T, G, aset = case.make_set(gpu, **kw)
        with pytest.raises(_lib.ZeroAmdError, match=f"zs_adamset_run_ema: .*{text}") as e:
            aset.run_ema(hp, 0.5, st)
        assert e.value.code == _lib.ZS_ERR_INVALID
        torch.cuda.synchronize()
        for name, ref in case.init.items():
            assert np.array_equal(T[name].cpu().numpy().view(np.uint8), ref.view(np.uint8)), name
    T, G, aset = case.make_set(gpu)
    for bad in (float("nan"), -0.5, 1.5):
        with pytest.raises(_lib.ZeroAmdError, match="ema_weight"):
            aset.run_ema(hp, bad, st)
    with pytest.raises(_lib.ZeroAmdError, match="guard"):
        aset.run_ema(hp, 0.5, st, guard=True)
