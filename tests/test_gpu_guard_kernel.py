"""The guarded update (zs_adamset_run_guarded, zs_adamset_run_sr_guarded) and zs_clip_coef_guarded.

The GUARD instances are the CLIP instances plus one uniform test of the coefficient, so two things
are pinned, over fp32 parameters with fp32 gradients, the split master with bf16 and with fp32
gradients, and bf16 moments rounded to nearest and stochastically (amsgrad on the fp32-state ones):

* with a finite coefficient every array the set points to has the bits the unguarded clipped run
  leaves from the same initial state;
* with the NaN coefficient every array is byte-identical to before, whatever the gradients hold.

Each set has a segment of two full chunks + 12 + 3 elements (full chunks, the predicated last
chunk, a scalar tail), a 5-element segment and a segment without a gradient.  The coefficient
kernel is compared bit for bit with a numpy restatement of include/zero_amd.h.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import zero_oracle as zo
from test_gpu_gradnorm import _coef_ref, _layout

pytestmark = pytest.mark.gpu

QNAN = 0x7FC00000
CONFIGS = {  # name: (split master, fp32 gradients, bf16 state, stochastic)
    "f32": (False, True, False, False),
    "split_bf16g": (True, False, False, False),
    "split_f32g": (True, True, False, False),
    "bf16state": (True, False, True, False),
    "bf16state_sr": (True, False, True, True),
}
CASES = [(c, False) for c in CONFIGS] + [(c, True) for c in CONFIGS if not CONFIGS[c][2]]
IDS = [c + ("-amsgrad" if a else "") for c, a in CASES]


def _segs(split):
    chunk = 4096 if split else 2048
    return _layout([2 * chunk + 12 + 3, 5, 2 * chunk + 12 + 3], no_grad=(2,))


def _bf16(x):
    return zo.f32_to_bf16_bits(np.ascontiguousarray(x, np.float32)).view(np.int16)


class _Set:
    """An Adam set of one configuration over host arrays ``init`` (name -> numpy), on the GPU."""

    def __init__(self, gpu, config, ams, init, segs):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import AdamSet

        split, g32, s16, self.sr = CONFIGS[config]
        self.T = T = {k: torch.from_numpy(v.copy()).to(gpu) for k, v in init.items()}
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in segs:
            g = at("g", o) if has_g else 0
            row = [g, at("hi", o), at("lo", o), at("hi", o)] if split else [g, at("p", o), at("p", o), 0]
            rows.append(row + [at("m", o), at("v", o), at("vmax", o), 0, n])
        self.aset = AdamSet(np.array(rows, np.uint64), ZS_F32 if g32 else ZS_BF16,
                            ZS_BF16_SPLIT if split else ZS_BF16, wide_grads=split and g32,
                            state_dtype=ZS_BF16 if s16 else None)
        self.ams = ams
        self.coef = torch.zeros(1, device=gpu)
        self.stream = torch.cuda.current_stream()

    def run(self, coef_bits, guard):
        from zero_amd.kernels import adam_hparams, sr_keys

        self.coef.copy_(torch.from_numpy(np.array([coef_bits], np.uint32).view(np.float32)))
        hp = adam_hparams(1e-3, 0.9, 0.99, 1e-8, 1e-2, 3, decoupled=True, amsgrad=self.ams,
                          grad_div=2.0)
        if self.sr:
            self.aset.run_sr(hp, self.T["m"].data_ptr(), sr_keys(11, 3), self.stream,
                             coef=self.coef, guard=guard)
        elif guard:
            self.aset.run_guarded(hp, self.coef, self.stream)
        else:
            self.aset.run_clipped(hp, self.coef, self.stream)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().view(np.uint8).copy() for k, v in self.T.items()}


def _init(config, ams, segs, rng, special=False):
    """Host arrays of one configuration: random state everywhere (also outside the segments, so a
    store past a segment shows); ``special``: NaN and +-inf among the gradients."""
    split, g32, s16, _ = CONFIGS[config]
    N = max(o + n for o, n, _ in segs) + 64
    g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
    if special:
        for o, n, has_g in segs:
            if has_g:
                k = min(n, 5)
                g[o:o + k] = np.array([np.nan, np.inf, -np.inf, 1.0, np.nan], np.float32)[:k]
                g[o + n - 1] = np.inf
    m = (rng.standard_normal(N) * 1e-2).astype(np.float32)
    v = (rng.standard_normal(N) ** 2 * 1e-4).astype(np.float32)
    out = {"g": g if g32 else _bf16(g), "m": _bf16(m) if s16 else m, "v": _bf16(v) if s16 else v}
    if ams:
        out["vmax"] = (v * np.float32(1.5)).astype(np.float32)
    p = (rng.standard_normal(N) * 0.05).astype(np.float32)
    if split:
        out["hi"] = _bf16(p)
        out["lo"] = rng.integers(-32768, 32768, N).astype(np.int16)
    else:
        out["p"] = p
    return out


@pytest.mark.parametrize("coef", [1.0, 0.3])
@pytest.mark.parametrize("config,ams", CASES, ids=IDS)
def test_finite_coefficient_equals_the_clipped_run(gpu, config, ams, coef):
    segs = _segs(CONFIGS[config][0])
    init = _init(config, ams, segs, np.random.default_rng(5))
    bits = int(np.float32(coef).view(np.uint32))
    want = _Set(gpu, config, ams, init, segs).run(bits, guard=False)
    got = _Set(gpu, config, ams, init, segs).run(bits, guard=True)
    changed = False
    for name in want:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, f"{name}: {bad.size} bytes differ, first at {bad[:4]}"
        changed = changed or not np.array_equal(want[name], init[name].view(np.uint8))
    assert changed, "the clipped run itself changed nothing"


@pytest.mark.parametrize("special", [False, True], ids=["ordinary", "nan-inf"])
@pytest.mark.parametrize("config,ams", CASES, ids=IDS)
def test_nan_coefficient_changes_nothing(gpu, config, ams, special):
    segs = _segs(CONFIGS[config][0])
    init = _init(config, ams, segs, np.random.default_rng(6), special)
    got = _Set(gpu, config, ams, init, segs).run(QNAN, guard=True)
    for name in got:
        bad = np.flatnonzero(got[name] != init[name].view(np.uint8))
        assert bad.size == 0, f"{name}: {bad.size} bytes changed, first at {bad[:4]}"


def _guarded_ref(sumsq, div, max_norm):
    """zs_clip_coef_guarded restated: zs_clip_coef's formulas (test_gpu_gradnorm._coef_ref), and
    the quiet NaN for a norm that is not finite.  Returns (two uint32 words, skipped?)."""
    out = _coef_ref(sumsq, div, max_norm).view(np.uint32).copy()
    skip = not np.isfinite(out[:1].view(np.float32)[0])
    if skip:
        out[1] = QNAN
    return out, skip


def test_guarded_coefficient_bits_and_counter(gpu):
    from zero_amd.kernels import clip_coef

    st = torch.cuda.current_stream()
    sumsq = torch.zeros(1, device=gpu)
    out2 = torch.zeros(2, device=gpu)
    skipped = torch.full((1,), 7, dtype=torch.int64, device=gpu)
    fmax = float(np.finfo(np.float32).max)
    want_count = 7
    for s in (0.0, 1e-30, 1.0, fmax, float("inf"), float("nan")):
        for m in (0.0, 1.0, float("inf")):
            for div in (1.0, 2.0):
                sumsq.fill_(s)
                plain = torch.zeros(2, device=gpu)
                clip_coef(sumsq, div, m, plain, st)
                clip_coef(sumsq, div, m, out2, st, skipped=skipped)
                torch.cuda.synchronize()
                got = out2.cpu().numpy().view(np.uint32)
                want, skip = _guarded_ref(np.float32(s), div, m)
                want_count += int(skip)
                what = f"sumsq {s!r} max_norm {m!r} grad_div {div!r}"
                if np.isnan(np.float32(s)):  # a NaN norm: any NaN payload is the norm as computed
                    assert np.isnan(got[:1].view(np.float32)[0]), what
                else:
                    assert got[0] == want[0], what
                assert got[1] == want[1], f"{what}: coef {got[1]:#x} want {want[1]:#x}"
                if not skip:  # a finite norm: zs_clip_coef's bits, never NaN
                    assert np.array_equal(got, plain.cpu().numpy().view(np.uint32)), what
                    assert not np.isnan(got[1:].view(np.float32)[0]), what
                assert int(skipped.item()) == want_count, what
    assert want_count == 7 + 2 * 3 * 2  # inf and NaN, every limit and divisor


def test_guarded_run_refuses_sgd_and_carry(gpu):
    from zero_amd import _lib
    from zero_amd.kernels import AdamSet, SgdSet, adam_hparams, sgd_hparams

    st = torch.cuda.current_stream()
    T = {k: torch.zeros(64, device=gpu) for k in ("g", "p", "m", "v", "c")}
    coef = torch.ones(1, device=gpu)
    ptr = lambda k: T[k].data_ptr()  # noqa: E731
    hp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    sgd = SgdSet(np.array([[ptr("g"), ptr("p"), ptr("p"), 0, ptr("m"), 0, 0, 0, 64]], np.uint64),
                 _lib.ZS_F32)
    with pytest.raises(_lib.ZeroAmdError):
        sgd.run_guarded(sgd_hparams(1e-2, 0.9), coef, st)
    rc = _lib.lib.zs_adamset_run_guarded(sgd._h, ctypes.byref(hp), coef.data_ptr(),
                                         int(st.cuda_stream))
    assert rc == _lib.ZS_ERR_INVALID and b"zs_adamset_run_guarded" in _lib.lib.zs_last_error()
    carry = AdamSet(np.array([[ptr("g"), ptr("p"), ptr("p"), 0, ptr("m"), ptr("v"), 0, ptr("c"), 64]],
                             np.uint64), _lib.ZS_F32)
    with pytest.raises(_lib.ZeroAmdError, match="carry"):
        carry.run_guarded(hp, coef, st)
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "c"):
        assert not T[k].any(), k
