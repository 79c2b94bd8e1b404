"""Fused Adam and SGD sets with ``ZS_F32`` gradients over the ``ZS_BF16_SPLIT`` master (what ZeRO-3
runs after an fp32-accumulated step), bit for bit against tests/_accum32_oracle.py's composition
of the existing oracles: join the split master, the fp32 update, split again.

Every case runs 3 steps with ``adam_loads_first`` at 0 and at 1 and compares every array the
kernels may write, whole (gaps between segments and the slack behind the last one included).  A NaN
need only be a NaN.  The chunk of the split-master instances is 4,096 elements.
"""
import numpy as np
import pytest
import torch

import _accum32_oracle as a32
import _sgd_oracle as so
from oracle import c_oracle

pytestmark = pytest.mark.gpu

C = 4096
STEPS = 3
SLACK = 4096
TIES = np.array([0x3C808000, 0x3C818000, 0xBC808000, 0xBC818000, 0x00008000, 0x80008000,
                 0x7F7F7FFF, 0x7F7F8000, 0x3F80FFFF, 0x00000000], np.uint32)
# (elements, has a gradient, elements off 16-byte alignment)
SPEC = [(C, True, 0),               # one full chunk
        (C + 1028, True, 0),        # a full chunk, then a partial one: a group and four elements
        (60, True, 0),              # shorter than one group
        (C + 4, False, 0),          # g == 0: weight decay and the moments still move it
        (C + 1028 + 3, True, 0),    # the same with a 3-element scalar tail
        (60, True, 1),              # misaligned: the scalar table only
        (3, True, 0),               # shorter than one vector access
        (2 * C + 8, True, 0)]


def _tune(key, value):
    from zero_amd import _lib

    _lib.call("zs_tune", key, int(value), None)


def _layout(spec):
    segs, off = [], 0
    for n, has_g, shift in spec:
        off = (off + 3) // 4 * 4 + shift
        segs.append((off, n, has_g))
        off += n
    return segs


SEGS = _layout(SPEC)
N = max(o + n for o, n, _ in SEGS) + SLACK


def _inputs(seed, specials=False):
    rng = np.random.default_rng(seed)
    master = (rng.standard_normal(N) * 0.02).astype(np.float32)
    u = master.view(np.uint32)
    for o, n, _ in SEGS:
        for at in (o, o + C):
            k = max(0, min(len(TIES), o + n - at))
            u[at:at + k] = TIES[:k]
    grads = []
    for _ in range(STEPS):
        g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
        # not bf16-representable: the low 16 bits are live
        assert ((g.view(np.uint32) & 0xFFFF) != 0).mean() > 0.99
        if specials:
            for o, n, has_g in SEGS:
                if has_g and n >= 60:
                    g[o + 5], g[o + 17], g[o + 29] = np.nan, np.inf, -np.inf
                    g[o + n - 1] = np.nan
        grads.append(g)
    return master, grads


def _reference(master, grads, kind, cfg, ws, rounded=False):
    """``rounded``: the bf16-gradient oracle on the gradients rounded to bf16."""
    hi, lo = c_oracle.split_master(master)
    out = {"hi": hi, "lo": lo, "m": np.zeros(N, np.float32)}
    ams = bool(cfg.get("amsgrad"))
    if kind == "adam":
        out["v"] = np.zeros(N, np.float32)
        if ams:
            out["vmax"] = np.zeros(N, np.float32)
    for t in range(1, STEPS + 1):
        for o, n, has_g in SEGS:
            sl = slice(o, o + n)
            g = grads[t - 1][sl].copy() if has_g else np.zeros(n, np.float32)
            if kind == "adam":
                hp = c_oracle.hparams(step=t, grad_div=float(ws), **cfg)
                h, l, m, v = (out[k][sl].copy() for k in ("hi", "lo", "m", "v"))
                x = out["vmax"][sl].copy() if ams else None
                if rounded:
                    c_oracle.adam_bf16_split(h, l, so.f32_to_bf16_bits(g), m, v, hp, vmax=x)
                else:
                    a32.adam_f32grad_split(h, l, g, m, v, hp, vmax=x)
                out["hi"][sl], out["lo"][sl], out["m"][sl], out["v"][sl] = h, l, m, v
                if ams:
                    out["vmax"][sl] = x
            else:
                hp = so.SgdHP(first=t == 1, grad_div=float(ws), **cfg)
                mom = cfg.get("momentum", 0.0) != 0
                buf = out["m"][sl].copy() if mom else None
                if rounded:
                    h, l, buf, _ = so.step_split(out["hi"][sl], out["lo"][sl],
                                                 so.f32_to_bf16_bits(g), buf, hp)
                else:
                    h, l, buf = a32.sgd_f32grad_split(out["hi"][sl], out["lo"][sl], g, buf, hp)
                out["hi"][sl], out["lo"][sl] = h, l
                if mom:
                    out["m"][sl] = buf
    return out


def _run_gpu(gpu, master, grads, kind, cfg, ws, lf, g_bf16=False, coef=None):
    """``coef``: run clipped, with this coefficient read from device memory."""
    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
    from zero_amd.kernels import AdamSet, SgdSet, adam_hparams, sgd_hparams

    hi0, lo0 = c_oracle.split_master(master)
    T = {"hi": torch.from_numpy(hi0.view(np.int16).copy()).to(gpu),
         "lo": torch.from_numpy(lo0.view(np.int16).copy()).to(gpu),
         "m": torch.zeros(N, device=gpu)}
    ams = bool(cfg.get("amsgrad"))
    if kind == "adam":
        T["v"] = torch.zeros(N, device=gpu)
        if ams:
            T["vmax"] = torch.zeros(N, device=gpu)
    G = torch.zeros(N, dtype=torch.int16 if g_bf16 else torch.float32, device=gpu)
    at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
    rows = []
    for o, n, has_g in SEGS:
        assert 0 <= o and o + n <= N - SLACK
        g = G.data_ptr() + o * G.element_size() if has_g else 0
        if kind == "adam":
            rows.append([g, at("hi", o), at("lo", o), at("hi", o), at("m", o), at("v", o),
                         at("vmax", o), 0, n])
        else:
            mom = cfg.get("momentum", 0.0) != 0
            rows.append([g, at("hi", o), at("lo", o), at("hi", o), at("m", o) if mom else 0, 0, 0, 0, n])
    rows = np.array(rows, dtype=np.uint64)
    mk = AdamSet if kind == "adam" else SgdSet
    aset = mk(rows, ZS_BF16 if g_bf16 else ZS_F32, ZS_BF16_SPLIT, wide_grads=not g_bf16)
    if not g_bf16:  # zs_adamset_stats: 28 B per element (Adam), 20 with momentum and 12 without
        per = (28 + (8 if ams else 0)) if kind == "adam" else \
            (20 if cfg.get("momentum", 0.0) != 0 else 12)
        n_g = sum(n for _, n, has_g in SEGS if has_g)
        n_all = sum(n for _, n, _ in SEGS)
        assert aset.elems == n_all and aset.bytes == per * n_all - 4 * (n_all - n_g)
    st = torch.cuda.current_stream()
    coef_t = None if coef is None else torch.full((1,), coef, device=gpu)
    run = aset.run if coef is None else lambda hp, st: aset.run_clipped(hp, coef_t, st)
    _tune(b"adam_loads_first", lf)
    try:
        for t in range(1, STEPS + 1):
            g = grads[t - 1]
            G.copy_(torch.from_numpy(so.f32_to_bf16_bits(g).view(np.int16) if g_bf16 else g))
            if kind == "adam":
                c = dict(cfg)
                run(adam_hparams(c.pop("lr", 1e-3), c.pop("beta1", 0.9), c.pop("beta2", 0.999),
                                 c.pop("eps", 1e-8), c.pop("weight_decay", 0.0), t,
                                 grad_div=float(ws), **c), st)
            else:
                run(sgd_hparams(first=t == 1, grad_div=float(ws), **cfg), st)
        torch.cuda.synchronize()
    finally:
        _tune(b"adam_loads_first", 1)
    out = {k: v.cpu().numpy() for k, v in T.items()}
    out["hi"], out["lo"] = out["hi"].view(np.uint16), out["lo"].view(np.uint16)
    return out, aset, G


def _compare(got, want, what):
    assert set(got) == set(want)
    pw, pg = c_oracle.join_master(want["hi"], want["lo"]), c_oracle.join_master(got["hi"], got["lo"])
    nan_p = np.isnan(pw)
    assert np.array_equal(np.isnan(pg), nan_p), f"{what}: master NaN where a number was wanted"
    for name, ref in want.items():
        g = got[name]
        if ref.dtype == np.float32:
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(g), nan), f"{what}: {name} NaN mismatch"
            bad = np.flatnonzero((g.view(np.uint32) != ref.view(np.uint32)) & ~nan)
        else:
            bad = np.flatnonzero((g != ref) & ~nan_p)
        assert bad.size == 0, f"{what}: {name}: {bad.size} elements differ, first at {bad[:8]}"


ADAM_CASES = {
    "default": dict(),
    "amsgrad": dict(amsgrad=True),
    "wd": dict(weight_decay=1e-2),
    "adamw_maximize": dict(weight_decay=1e-2, decoupled=True, maximize=True),
    "amsgrad_hyper": dict(amsgrad=True, lr=1e-2, beta1=0.4, beta2=0.99, eps=1e-6, maximize=True),
}
SGD_CASES = {
    "plain": dict(lr=0.05),
    "momentum_wd": dict(lr=0.05, momentum=0.9, weight_decay=1e-2),
    "nesterov": dict(lr=0.05, momentum=0.9, nesterov=True, maximize=True),
}


@pytest.mark.parametrize("case", list(ADAM_CASES))
def test_adam_sets(gpu, case):
    cfg = ADAM_CASES[case]
    ws = 3 if "hyper" in case else 2
    master, grads = _inputs(21)
    want = _reference(master, grads, "adam", cfg, ws)
    for lf in (0, 1):
        got, _, _ = _run_gpu(gpu, master, grads, "adam", cfg, ws, lf)
        _compare(got, want, f"adam {case} adam_loads_first={lf}")


@pytest.mark.parametrize("case", list(SGD_CASES))
def test_sgd_sets(gpu, case):
    cfg = SGD_CASES[case]
    master, grads = _inputs(22)
    want = _reference(master, grads, "sgd", cfg, 3)
    for lf in (0, 1):
        got, _, _ = _run_gpu(gpu, master, grads, "sgd", cfg, 3, lf)
        # (without momentum the set has no buffer: "m" stays this test's zeros on both sides)
        _compare(got, want, f"sgd {case} adam_loads_first={lf}")


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_nan_and_inf_gradients(gpu, kind):
    cfg = dict(amsgrad=True) if kind == "adam" else dict(lr=0.05, momentum=0.9)
    master, grads = _inputs(23, specials=True)
    want = _reference(master, grads, kind, cfg, 2)
    assert np.isnan(want["m"]).any() and not np.isnan(want["m"]).all()
    for lf in (0, 1):
        got, _, _ = _run_gpu(gpu, master, grads, kind, cfg, 2, lf)
        _compare(got, want, f"{kind} specials adam_loads_first={lf}")


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_the_gradient_is_read_as_fp32(gpu, kind):
    """The same gradients rounded to bf16 through the bf16-gradient set give another result: a set
    that rounded its fp32 gradients on the way in could not pass the cases above by accident."""
    cfg = dict() if kind == "adam" else dict(lr=0.05, momentum=0.9)
    master, grads = _inputs(24)
    got32, _, _ = _run_gpu(gpu, master, grads, kind, cfg, 2, 1)
    got16, _, _ = _run_gpu(gpu, master, grads, kind, cfg, 2, 1, g_bf16=True)
    _compare(got16, _reference(master, grads, kind, cfg, 2, rounded=True), f"{kind} rounded")
    assert (got32["m"].view(np.uint32) != got16["m"].view(np.uint32)).any()
    assert (got32["lo"] != got16["lo"]).any()


def test_grad_sqnorm_within_the_split_bound(gpu):
    """(K + 2) * 2^-24 relative with K = 16 fp32 terms per lane and chunk, against
    float64, with both cache policies."""
    from zero_amd.kernels import sqnorm_reduce

    master, grads = _inputs(25)
    _, aset, G = _run_gpu(gpu, master, grads, "adam", dict(), 2, 1)
    g = grads[-1].astype(np.float64)
    want = sum(float((g[o:o + n] ** 2).sum()) for o, n, has_g in SEGS if has_g)
    assert aset.grad_bytes == 4 * sum(n for _, n, has_g in SEGS if has_g)
    st = torch.cuda.current_stream()
    for nt in (1, 0):
        _tune(b"sqnorm_nt", nt)
        try:
            partials = torch.full((aset.sqnorm_partials,), float("nan"), dtype=torch.float64, device=gpu)
            sumsq = torch.zeros(1, device=gpu)
            aset.grad_sqnorm(partials, st)
            sqnorm_reduce(partials, aset.sqnorm_partials, sumsq, st)
            torch.cuda.synchronize()
        finally:
            _tune(b"sqnorm_nt", 1)
        rel = abs(float(sumsq.item()) - want) / want
        print(f"sqnorm_nt={nt}: sumsq {float(sumsq.item())!r} vs float64 {want!r}: rel {rel:.3e}")
        assert np.isfinite(float(sumsq.item())) and rel <= (16 + 2) * 2.0 ** -24


def test_clipped_run_equals_the_pre_scaled_gradient(gpu):
    """zs_adamset_run_clipped on such a set: coefficient 0.5 on g equals the plain run on 0.5 * g
    (a power of two: the product is exact either way)."""
    from zero_amd._lib import ZS_BF16_SPLIT, ZS_F32
    from zero_amd.kernels import AdamSet, adam_hparams

    rng = np.random.default_rng(26)
    n = 2 * C + 1028 + 3
    master = (rng.standard_normal(n) * 0.02).astype(np.float32)
    g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    hi0, lo0 = c_oracle.split_master(master)
    outs = []
    for clipped in (True, False):
        hi = torch.from_numpy(hi0.view(np.int16).copy()).to(gpu)
        lo = torch.from_numpy(lo0.view(np.int16).copy()).to(gpu)
        m, v, x = (torch.zeros(n, device=gpu) for _ in range(3))
        G = torch.from_numpy(g if clipped else g * np.float32(0.5)).to(gpu)
        rows = np.array([[G.data_ptr(), hi.data_ptr(), lo.data_ptr(), hi.data_ptr(), m.data_ptr(),
                          v.data_ptr(), x.data_ptr(), 0, n]], np.uint64)
        aset = AdamSet(rows, ZS_F32, ZS_BF16_SPLIT, wide_grads=True)
        coef = torch.full((1,), 0.5, device=gpu)
        st = torch.cuda.current_stream()
        for t in (1, 2):
            hp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 1e-2, t, amsgrad=True, grad_div=2.0)
            if clipped:
                aset.run_clipped(hp, coef, st)
            else:
                aset.run(hp, st)
        torch.cuda.synchronize()
        outs.append([t_.cpu().numpy() for t_ in (hi, lo, m, v, x)])
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # and the C oracle on the halved gradient
    h, l = hi0.copy(), lo0.copy()
    m, v, x = (np.zeros(n, np.float32) for _ in range(3))
    for t in (1, 2):
        a32.adam_f32grad_split(h, l, g * np.float32(0.5), m, v,
                               c_oracle.hparams(step=t, weight_decay=1e-2, amsgrad=True, grad_div=2.0),
                               vmax=x)
    assert np.array_equal(outs[0][0].view(np.uint16), h) and np.array_equal(outs[0][1].view(np.uint16), l)
    assert np.array_equal(outs[0][4].view(np.uint32), x.view(np.uint32))


CLIPPED_CASES = {
    "adam": ("adam", dict(weight_decay=1e-2)),
    "adam_amsgrad": ("adam", dict(amsgrad=True, weight_decay=1e-2)),
    "sgd": ("sgd", dict(lr=0.05, weight_decay=1e-2)),
    "sgd_momentum": ("sgd", dict(lr=0.05, momentum=0.9, weight_decay=1e-2)),
}


@pytest.mark.parametrize("case", list(CLIPPED_CASES))
def test_clipped_instances(gpu, case):
    """Every clipped instance of these sets, with and without amsgrad / a momentum buffer, with
    ``adam_loads_first`` at 0 and at 1, over the full and partial chunks, the scalar tails and the
    segment without a gradient of SPEC: coefficient 0.5 on g (a power of two, as grad_div = 2: both
    products are exact) equals the oracle on 0.5 * g."""
    kind, cfg = CLIPPED_CASES[case]
    master, grads = _inputs(27)
    want = _reference(master, [g * np.float32(0.5) for g in grads], kind, cfg, 2)
    for lf in (0, 1):
        got, _, _ = _run_gpu(gpu, master, grads, kind, cfg, 2, lf, coef=0.5)
        _compare(got, want, f"clipped {case} adam_loads_first={lf}")


def test_refusals(gpu):
    from zero_amd._lib import ZS_BF16_SPLIT, ZS_ERR_INVALID, ZS_F32, ZeroAmdError
    from zero_amd.kernels import AdamSet, SgdSet, adam_hparams, sgd_hparams

    n = 64
    hi = torch.zeros(n, dtype=torch.bfloat16, device=gpu)
    lo = torch.zeros(n, dtype=torch.int16, device=gpu)
    g, m, v, cr = (torch.zeros(n, device=gpu) for _ in range(4))
    row = lambda carry, vv: np.array([[g.data_ptr(), hi.data_ptr(), lo.data_ptr(), hi.data_ptr(),  # noqa: E731
                                       m.data_ptr(), vv, 0, carry, n]], np.uint64)
    for mk, vv in ((AdamSet, v.data_ptr()), (SgdSet, 0)):
        with pytest.raises(ZeroAmdError, match="bf16 grads") as e:  # fp32 grads only by name
            mk(row(0, vv), ZS_F32, ZS_BF16_SPLIT)
        assert e.value.code == ZS_ERR_INVALID
        with pytest.raises(ZeroAmdError, match="no carry") as e:
            mk(row(cr.data_ptr(), vv), ZS_F32, ZS_BF16_SPLIT, wide_grads=True)
        assert e.value.code == ZS_ERR_INVALID
    st = torch.cuda.current_stream()
    aset = AdamSet(row(0, v.data_ptr()), ZS_F32, ZS_BF16_SPLIT, wide_grads=True)
    sset = SgdSet(row(0, 0), ZS_F32, ZS_BF16_SPLIT, wide_grads=True)
    with pytest.raises(ZeroAmdError, match="zs_sgdset_create") as e:  # an SGD set, the Adam call
        AdamSet.run(sset, adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1), st)
    assert e.value.code == ZS_ERR_INVALID
    with pytest.raises(ZeroAmdError, match="zs_adamset_create") as e:  # an Adam set, the SGD call
        SgdSet.run(aset, sgd_hparams(0.1), st)
    assert e.value.code == ZS_ERR_INVALID
    torch.cuda.synchronize()
    assert not hi.float().any() and not m.any()  # nothing ran
