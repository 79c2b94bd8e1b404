"""Global gradient-norm clipping at the kernel level: the sum-of-squares pass over an Adam set, the
fixed-order reducer, the coefficient kernel and the CLIP instances of the fused Adam.

Every expected value comes from numpy in float64, the numpy restatement of the coefficient
formulas (include/zero_amd.h zs_clip_coef) or the C oracle; none from the code under test.  The
oracle has no clipping, so the clipped update is restated as the unclipped one on the pre-clipped
gradient g' = float32(float32(g) / div) * coef with grad_div = 1 (``_ref_step``);
``test_harness_matches_oracle`` pins that restatement against the oracle's own three entry points
on the CPU.  The Adam checks use the coefficient read back from the device, so they stay bitwise
and the coefficient is judged on its own.

C below is the chunk of the instance: 4,096 elements for the split master, 2,048 otherwise.  A lane
adds 4 elements per group and a chunk has C / 1024 groups, so the fp32 part of the sum is
K = 16 (split) or 8 terms; the bound on the fp32 ``sumsq`` is (K + 2) * 2^-24 relative: K roundings
of non-negative fmaf terms, the double levels above (negligible) and the final rounding to fp32.
"""
import ctypes

import numpy as np
import pytest

from oracle import c_oracle
from oracle import zero_oracle as zo

gpu_test = pytest.mark.gpu

KINDS = ("split", "bf16", "f32")  # bf16 grad + split master / bf16 grad + fp32 master / fp32 grad
CHUNK = {"split": 4096, "bf16": 2048, "f32": 2048}
TERMS = {"split": 16, "bf16": 8, "f32": 8}  # fp32 terms a lane adds per chunk
SLACK = 4096
POISON = np.float32(1e30)  # its square overflows fp32: one read outside a segment makes the norm inf
TIES = np.array([0x3C808000, 0x3C818000, 0xBC808000, 0xBC818000, 0x00008000, 0x80008000,
                 0x7F7F7FFF, 0x7F7F8000, 0x3F80FFFF, 0x00000000], np.uint32)


def _tune(key, value):
    from zero_amd import _lib

    _lib.call("zs_tune", key, int(value), None)


def _layout(lengths, no_grad=(), shifted=()):
    """Segments (offset, n, has_grad): 16-byte aligned with a gap of at least 4 elements between
    them; those in ``shifted`` start one element off alignment (the scalar path)."""
    segs, off = [], 0
    for k, n in enumerate(lengths):
        off = (off + 3) // 4 * 4 + 4 + (1 if k in shifted else 0)
        segs.append((off, n, k not in no_grad))
        off += n
    return segs


def _grad_array(kind, segs, rng, scale=1e-2):
    """Host gradient arena: random values inside the segments, POISON everywhere else."""
    N = max(o + n for o, n, _ in segs) + SLACK
    g = np.full(N, POISON, np.float32)
    for o, n, _ in segs:
        g[o:o + n] = (rng.standard_normal(n) * scale).astype(np.float32)
    return g if kind == "f32" else zo.f32_to_bf16_bits(g)


def _as_f64(kind, g):
    return (g if kind == "f32" else zo.bf16_bits_to_f32(g)).astype(np.float64)


def _sumsq64(kind, g, segs):
    x = _as_f64(kind, g)
    return float(sum(np.sum(x[o:o + n] ** 2) for o, n, has_g in segs if has_g))


class _Dev:
    """An Adam set over ``segs`` on the GPU with zeroed state (``master0``: fp32 initial master)."""

    def __init__(self, gpu, kind, segs, *, ams=False, carry=False, master0=None):
        import torch

        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import AdamSet

        self.kind, self.segs, self.gpu = kind, segs, gpu
        self.N = N = max(o + n for o, n, _ in segs) + SLACK
        if master0 is None:
            master0 = np.zeros(N, np.float32)
        T = {"m": torch.zeros(N, device=gpu), "v": torch.zeros(N, device=gpu)}
        if ams:
            T["vmax"] = torch.zeros(N, device=gpu)
        if carry:
            T["carry"] = torch.zeros(N, device=gpu)
        if kind == "split":
            hi0, lo0 = c_oracle.split_master(master0)
            T["hi"] = torch.from_numpy(hi0.view(np.int16).copy()).to(gpu)
            T["lo"] = torch.from_numpy(lo0.view(np.int16).copy()).to(gpu)
        else:
            T["p"] = torch.from_numpy(master0.copy()).to(gpu)
            if kind == "bf16":
                T["pb"] = torch.zeros(N, dtype=torch.int16, device=gpu)
        self.T = T
        self.gdt = torch.float32 if kind == "f32" else torch.int16
        self.G = torch.zeros(N, dtype=self.gdt, device=gpu)
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in segs:
            g = self.gptr(self.G, o) if has_g else 0
            if kind == "split":
                row = [g, at("hi", o), at("lo", o), at("hi", o)]
            else:
                row = [g, at("p", o), at("p", o), at("pb", o)]
            rows.append(row + [at("m", o), at("v", o), at("vmax", o), at("carry", o), n])
        self.aset = AdamSet(np.array(rows, dtype=np.uint64), ZS_F32 if kind == "f32" else ZS_BF16,
                            ZS_BF16_SPLIT if kind == "split" else ZS_BF16)
        self.partials = torch.full((self.aset.sqnorm_partials + 8,), -1.0, dtype=torch.float64,
                                   device=gpu)
        self.sumsq = torch.zeros(1, device=gpu)
        self.out2 = torch.zeros(2, device=gpu)
        self.stream = torch.cuda.current_stream()

    @staticmethod
    def gptr(G, o):
        return G.data_ptr() + o * G.element_size()

    def upload(self, g, G=None):
        import torch

        (self.G if G is None else G).copy_(torch.from_numpy(g if self.kind == "f32" else g.view(np.int16)))

    def norm(self):
        """The pass and the reducer; returns (partials as uint64 bits, sumsq as fp32)."""
        import torch

        from zero_amd.kernels import sqnorm_reduce

        self.partials.fill_(-1.0)
        self.aset.grad_sqnorm(self.partials, self.stream)
        sqnorm_reduce(self.partials, self.aset.sqnorm_partials, self.sumsq, self.stream)
        torch.cuda.synchronize()
        part = self.partials.cpu().numpy()
        n = self.aset.sqnorm_partials
        assert (part[n:] == -1.0).all(), "a partial was written past the set's count"
        return part[:n].view(np.uint64).copy(), np.float32(self.sumsq.cpu().numpy()[0])

    def coef(self, max_norm, div):
        import torch

        from zero_amd.kernels import clip_coef

        clip_coef(self.sumsq, div, max_norm, self.out2, self.stream)
        torch.cuda.synchronize()
        return self.out2.cpu().numpy().copy()

    def arrays(self):
        return {k: v.cpu().numpy() for k, v in self.T.items()}


def _coef_ref(sumsq, div, max_norm):
    """The formulas of include/zero_amd.h zs_clip_coef, restated."""
    with np.errstate(all="ignore"):
        norm = np.float32(np.sqrt(np.float64(np.float32(sumsq))) / np.float64(div))
        c = np.float32(max_norm) / np.float32(norm + np.float32(1e-6))
        coef = np.float32(1.0) if c > np.float32(1.0) else np.float32(c)
    return np.array([norm, coef], np.float32)


def _check_sumsq(kind, got, want):
    assert np.isfinite(got), "the pass read outside a segment (or overflowed)"
    bound = (TERMS[kind] + 2) * 2.0 ** -24
    rel = abs(float(got) - want) / want
    print(f"{kind}: sumsq {got!r} vs float64 {want!r}: rel {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound


# ---------------------------------------------------------------------------------------------
# the norm against float64
# ---------------------------------------------------------------------------------------------
def _tables(kind):
    C = CHUNK[kind]
    return {
        # full chunks, a partial chunk, a scalar tail
        "one": _layout([2 * C + 4 * 37 + 3]),
        # one segment without a gradient, one starting one element off alignment
        "mixed": _layout([1, 3, 4, 255, 1024, C - 4, C, C + 4, 3 * C + 1028], no_grad=(6,),
                         shifted=(4,)),
    }


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("table", ["one", "mixed"])
def test_norm_against_float64(gpu, kind, table):
    segs = _tables(kind)[table]
    g = _grad_array(kind, segs, np.random.default_rng(5))
    d = _Dev(gpu, kind, segs)
    d.upload(g)
    _, ss = d.norm()
    _check_sumsq(kind, ss, _sumsq64(kind, g, segs))


PARTIALS_CAP = 8192  # partials (= workgroups) of a set's vector table at the most


@gpu_test
@pytest.mark.parametrize("kind", ["split", "f32"])
def test_norm_workgroup_strides_over_chunks(gpu, kind):
    """A few more chunks than the set has partials: workgroups 0..5 sum two chunks each."""
    C = CHUNK[kind]
    assert _Dev(gpu, kind, _layout([3 * C])).aset.sqnorm_partials == 3
    cap = PARTIALS_CAP
    segs = _layout([(cap + 5) * C + 8])
    g = _grad_array(kind, segs, np.random.default_rng(6))
    d = _Dev(gpu, kind, segs)
    assert d.aset.sqnorm_partials == cap
    d.upload(g)
    _, ss = d.norm()
    _check_sumsq(kind, ss, _sumsq64(kind, g, segs))


SCALAR_PARTIALS_CAP = 1024  # partials (= workgroups) of a set's scalar table at the most


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
def test_norm_scalar_table_strides_over_chunks(gpu, kind):
    """A scalar table of 1,029 chunks of 256 elements against its 1,024 partials: workgroups 0..4
    sum two chunks each, and the scan of workgroups 2..4 crosses from the first shifted segment
    into the second.  The aligned segment in front gives the vector table its one partial."""
    C = CHUNK[kind]
    segs = _layout([C, SCALAR_PARTIALS_CAP * 256 + 300, 700], shifted=(1, 2))
    sca_chunks = sum(-(-n // 256) for _, n, _ in segs[1:])
    assert sca_chunks == 1029 and sca_chunks > SCALAR_PARTIALS_CAP
    g = _grad_array(kind, segs, np.random.default_rng(12))
    d = _Dev(gpu, kind, segs)
    assert d.aset.sqnorm_partials == 1 + SCALAR_PARTIALS_CAP
    d.upload(g)
    _, ss = d.norm()
    _check_sumsq(kind, ss, _sumsq64(kind, g, segs))


@gpu_test
@pytest.mark.parametrize("kind", ["split", "f32"])
def test_norm_is_deterministic(gpu, kind):
    """Identical bits from run to run and under the Adam's knobs; after set_grads the norm is the
    new buffer's."""
    import torch

    segs = _tables(kind)["mixed"]
    rng = np.random.default_rng(8)
    g, g2 = _grad_array(kind, segs, rng), _grad_array(kind, segs, rng, scale=3e-2)
    d = _Dev(gpu, kind, segs)
    d.upload(g)
    p0, s0 = d.norm()
    p1, s1 = d.norm()
    assert np.array_equal(p0, p1) and s0.view(np.uint32) == s1.view(np.uint32)
    for key, value, back in ((b"adam_wg_per_cu", 7, 0), (b"adam_loads_first", 0, 1),
                             (b"sqnorm_nt", 0, 1)):
        _tune(key, value)
        try:
            pk, sk = d.norm()
        finally:
            _tune(key, back)
        assert np.array_equal(p0, pk) and s0.view(np.uint32) == sk.view(np.uint32), key
    G2 = torch.zeros_like(d.G)
    d.upload(g2, G2)
    d.aset.set_grads(np.array([_Dev.gptr(G2, o) if has_g else 0 for o, _, has_g in segs], np.uint64),
                     d.stream)
    _, s2 = d.norm()
    _check_sumsq(kind, s2, _sumsq64(kind, g2, segs))
    assert abs(float(s2) - float(s0)) > 0.5 * float(s0)  # the two buffers' norms are far apart


# ---------------------------------------------------------------------------------------------
# the coefficient, bit for bit
# ---------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("case", ["below", "above_div3", "inf", "zeros", "nan"])
def test_coefficient_bits(gpu, case):
    kind = "f32"
    C = CHUNK[kind]
    segs = _layout([C + 12, 7])
    g = _grad_array(kind, segs, np.random.default_rng(9))
    if case == "zeros":
        for o, n, _ in segs:
            g[o:o + n] = 0
    if case == "nan":
        g[segs[0][0] + C + 5] = np.nan
    d = _Dev(gpu, kind, segs)
    d.upload(g)
    _, ss = d.norm()
    norm64 = np.sqrt(_sumsq64(kind, g, segs))
    max_norm, div = {"below": (4.0 * norm64, 1.0), "above_div3": (0.1 * norm64 / 3.0, 3.0),
                     "inf": (float("inf"), 2.0), "zeros": (1.0, 1.0), "nan": (1.0, 1.0)}[case]
    got = d.coef(max_norm, div)
    want = _coef_ref(ss, div, max_norm)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    if case in ("below", "inf", "zeros"):
        assert got.view(np.uint32)[1] == 0x3F800000
    if case == "above_div3":
        assert abs(float(got[1]) - 0.1) < 1e-3
        assert abs(float(got[0]) - norm64 / 3.0) <= 1e-5 * norm64
    if case == "inf":
        assert abs(float(got[0]) - norm64 / 2.0) <= 1e-5 * norm64
    if case == "zeros":
        assert got[0] == 0.0
    if case == "nan":
        assert np.isnan(got[0]) and np.isnan(got[1])


# ---------------------------------------------------------------------------------------------
# the clipped update against the oracle
# ---------------------------------------------------------------------------------------------
SCALES = (1.0, 40.0, 0.05)  # per step: coefficient exactly 1, well below 1, exactly 1
VARIANTS = {"plain": dict(div=1.0), "amsgrad": dict(div=3.0, amsgrad=True),
            "adamw": dict(div=2.0, weight_decay=1e-2, decoupled=True)}


def _ref_step(kind, out, segs, g, div, coef, hp):
    """One clipped step of the reference: the unmodified oracle's fp32 update on the pre-clipped
    gradient g' = float32(float32(g) / div) * coef with grad_div = 1, the bf16 parameter and the
    split master derived from the fp32 result.  ``out`` is updated in place on the segments."""
    for o, n, has_g in segs:
        sl = slice(o, o + n)
        gf = (g[sl] if kind == "f32" else zo.bf16_bits_to_f32(g[sl])).astype(np.float32)
        if not has_g:
            gf = np.zeros(n, np.float32)
        with np.errstate(all="ignore"):
            gp = np.ascontiguousarray((gf / np.float32(div)).astype(np.float32) * np.float32(coef))
        p = c_oracle.join_master(out["hi"][sl], out["lo"][sl]) if kind == "split" else out["p"][sl].copy()
        m, v = out["m"][sl].copy(), out["v"][sl].copy()
        vmax = out["vmax"][sl].copy() if "vmax" in out else None
        c_oracle.adam_f32(p, gp, m, v, hp, vmax=vmax)
        out["m"][sl], out["v"][sl] = m, v
        if vmax is not None:
            out["vmax"][sl] = vmax
        if kind == "split":
            out["hi"][sl], out["lo"][sl] = c_oracle.split_master(p)
        else:
            out["p"][sl] = p
            if kind == "bf16":
                out["pb"][sl] = zo.f32_to_bf16_bits(p)


def _ref_init(kind, N, master0, ams):
    out = {"m": np.zeros(N, np.float32), "v": np.zeros(N, np.float32)}
    if ams:
        out["vmax"] = np.zeros(N, np.float32)
    if kind == "split":
        out["hi"], out["lo"] = c_oracle.split_master(master0)
    else:
        out["p"] = master0.copy()
        if kind == "bf16":
            out["pb"] = np.zeros(N, np.uint16)
    return out


def _master(N, segs, C, rng):
    master0 = (rng.standard_normal(N) * 0.02).astype(np.float32)
    u = master0.view(np.uint32)
    for o, n, _ in segs:  # every tie class of the split encoding at the head of each segment
        k = min(len(TIES), n)
        u[o:o + k] = TIES[:k]
    return master0


def _bits(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint16)


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_clipped_adam_bitwise(gpu, kind, variant):
    """3 steps of norm -> coefficient -> clipped update with gradient scales x1, x40, x0.05, under
    both adam_loads_first settings, every array whole (gaps and slack included) against the oracle
    run with the coefficient the device reported."""
    C = CHUNK[kind]
    _clipped_case(gpu, kind, variant,
                  _layout([2 * C + 4 * 37 + 3, C + 8, 300], no_grad=(1,), shifted=(2,)))


def _clipped_case(gpu, kind, variant, segs, wg_per_cu=0):
    import torch

    from zero_amd.kernels import adam_hparams

    C = CHUNK[kind]
    v = dict(VARIANTS[variant])
    div, ams = v.pop("div"), v.get("amsgrad", False)
    rng = np.random.default_rng(31)
    N = max(o + n for o, n, _ in segs) + SLACK
    master0 = _master(N, segs, C, rng)
    grads = [_grad_array(kind, segs, rng, scale=1e-2 * s) for s in SCALES]
    max_norm = 4.0 * np.sqrt(_sumsq64(kind, grads[0], segs)) / div
    results = {}
    for lf in (0, 1):
        d = _Dev(gpu, kind, segs, ams=ams, master0=master0)
        coefs = []
        _tune(b"adam_loads_first", lf)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            for t, g in enumerate(grads, 1):
                d.upload(g)
                d.norm()
                coefs.append(d.coef(max_norm, div))
                hp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, v.get("weight_decay", 0.0), t,
                                  decoupled=v.get("decoupled", False), amsgrad=ams, grad_div=div)
                d.aset.run_clipped(hp, d.out2.data_ptr() + 4, d.stream)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        results[lf] = (d.arrays(), coefs)
    coefs = results[1][1]
    for a, b in zip(results[0][1], coefs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    print("coefficients", [float(c[1]) for c in coefs])
    assert coefs[0].view(np.uint32)[1] == 0x3F800000 and coefs[2].view(np.uint32)[1] == 0x3F800000
    assert 0.05 < coefs[1][1] < 0.2
    want = _ref_init(kind, N, master0, ams)
    for t, g in enumerate(grads, 1):
        hp = c_oracle.hparams(step=t, weight_decay=v.get("weight_decay", 0.0),
                              decoupled=v.get("decoupled", False), amsgrad=ams, grad_div=1.0)
        _ref_step(kind, want, segs, g, div, coefs[t - 1][1], hp)
    for lf in (0, 1):
        got = results[lf][0]
        for name, ref in want.items():
            bad = np.flatnonzero(_bits(got[name]) != _bits(ref))
            assert bad.size == 0, (f"{name}, adam_loads_first={lf}: {bad.size} elements differ "
                                   f"from the oracle, first at {bad[:8]}")


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant", ["plain", "amsgrad"])
def test_clipped_scalar_table_strides_past_the_grid(gpu, kind, variant):
    """The same harness on a table whose scalar part has more than 2 * cus chunks, with one
    workgroup per CU: every workgroup of the clipped scalar instance goes round its stride loop at
    least twice and scans across all four entries (two long shifted segments around an aligned
    7-element one and a shifted one without a gradient)."""
    import torch

    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    lengths, shifted = [256 * cus + 300, 7, 300, 256 * cus + 513], (0, 2, 3)
    sca_chunks = sum(-(-(n if k in shifted else n % 4) // 256) for k, n in enumerate(lengths))
    assert sca_chunks == 2 * cus + 8 and sca_chunks > 2 * cus
    _clipped_case(gpu, kind, variant, _layout(lengths, no_grad=(2,), shifted=shifted), wg_per_cu=1)


@gpu_test
def test_clipped_run_refuses_carry(gpu):
    import torch

    from zero_amd._lib import ZS_ERR_INVALID, ZeroAmdError
    from zero_amd.kernels import adam_hparams

    kind = "f32"
    segs = _layout([CHUNK[kind] + 7])
    rng = np.random.default_rng(2)
    d = _Dev(gpu, kind, segs, carry=True, master0=_master(segs[0][0] + segs[0][1] + SLACK, segs, 0, rng))
    d.upload(_grad_array(kind, segs, rng))
    d.out2.fill_(0.5)
    before = d.arrays()
    with pytest.raises(ZeroAmdError) as e:
        d.aset.run_clipped(adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, grad_div=2.0, carry_mul=1.0),
                           d.out2.data_ptr() + 4, d.stream)
    assert e.value.code == ZS_ERR_INVALID and "carry" in str(e.value)
    torch.cuda.synchronize()
    after = d.arrays()
    for name in before:
        assert np.array_equal(_bits(before[name]), _bits(after[name])), name


# ---------------------------------------------------------------------------------------------
# CPU: the harness restatement and argument validation
# ---------------------------------------------------------------------------------------------
def test_harness_matches_oracle():
    """At coef = 1 the pre-clipped-gradient restatement equals the oracle's own fp32, bf16 and
    split-master entry points bit for bit (3 steps, 50,000 elements, every tie class, a divisor
    that is no power of two), so what ``_ref_step`` adds to the oracle is the multiply alone."""
    n, div = 50_000, 3.0
    segs = [(0, n, True)]
    for kind in KINDS:
        rng = np.random.default_rng(77)
        master0 = _master(n, [(o, 10, True) for o in range(0, n, 5000)], 0, rng)
        a = _ref_init(kind, n, master0, False)
        b = _ref_init(kind, n, master0, False)
        for t in (1, 2, 3):
            g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
            if kind != "f32":
                g = zo.f32_to_bf16_bits(g)
            _ref_step(kind, a, segs, g, div, 1.0, c_oracle.hparams(step=t, grad_div=1.0))
            hp = c_oracle.hparams(step=t, grad_div=div)
            if kind == "split":
                c_oracle.adam_bf16_split(b["hi"], b["lo"], g, b["m"], b["v"], hp)
            elif kind == "bf16":
                c_oracle.adam_bf16(b["p"], b["pb"], g, b["m"], b["v"], hp)
            else:
                c_oracle.adam_f32(b["p"], g, b["m"], b["v"], hp)
        for name in b:
            assert np.array_equal(_bits(a[name]), _bits(b[name])), (kind, name)


def test_coefficient_restatement_matches_torch():
    """The fp32 formula of ``_coef_ref`` is clip_grad_norm_'s: max_norm / (norm + 1e-6) clamped at 1."""
    import torch

    for sumsq, max_norm in ((6.3, 1.0), (0.09, 1.0), (0.0, 1.0), (49.5, float("inf")), (1e-3, 0.01)):
        norm = torch.tensor(float(np.float32(np.sqrt(np.float64(np.float32(sumsq))))), dtype=torch.float32)
        t = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        got = _coef_ref(sumsq, 1.0, max_norm)
        assert got[0] == np.float32(norm.item()) and got[1] == np.float32(t.item()), (sumsq, max_norm)


def test_argument_validation():
    """Null pointers, a negative or NaN limit and a non-positive divisor are ZS_ERR_INVALID before
    anything is launched (so without a GPU); an empty set has no partials."""
    from zero_amd import _lib
    from zero_amd._lib import AdamHParams, AdamSeg

    L, INV = _lib.lib, _lib.ZS_ERR_INVALID
    h = ctypes.c_void_p()
    _lib.call("zs_adamset_create", (AdamSeg * 1)(), 0, _lib.ZS_F32, _lib.ZS_BF16, ctypes.byref(h))
    try:
        n = ctypes.c_int64(-1)
        _lib.call("zs_adamset_sqnorm_partials", h, ctypes.byref(n))
        assert n.value == 0
        _lib.call("zs_adamset_grad_sqnorm", h, None, 0)  # empty set: nothing to write or launch
        hp = AdamHParams()
        fake = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its checks
        assert L.zs_adamset_sqnorm_partials(None, ctypes.byref(n)) == INV
        assert L.zs_adamset_sqnorm_partials(h, None) == INV
        assert L.zs_adamset_grad_sqnorm(None, fake, 0) == INV
        assert L.zs_sqnorm_reduce(None, 4, fake, 0) == INV
        assert L.zs_sqnorm_reduce(fake, 4, None, 0) == INV
        assert L.zs_sqnorm_reduce(fake, -1, fake, 0) == INV
        assert L.zs_clip_coef(None, 1.0, 1.0, fake, 0) == INV
        assert L.zs_clip_coef(fake, 1.0, 1.0, None, 0) == INV
        assert L.zs_clip_coef(fake, 1.0, -1.0, fake, 0) == INV
        assert L.zs_clip_coef(fake, 1.0, float("nan"), fake, 0) == INV
        assert L.zs_clip_coef(fake, 0.0, 1.0, fake, 0) == INV
        assert L.zs_clip_coef(fake, -2.0, 1.0, fake, 0) == INV
        assert L.zs_adamset_run_clipped(None, ctypes.byref(hp), fake, 0) == INV
        assert L.zs_adamset_run_clipped(h, None, fake, 0) == INV
        assert L.zs_adamset_run_clipped(h, ctypes.byref(hp), None, 0) == INV
        assert b"NULL" in L.zs_last_error()
    finally:
        _lib.call("zs_adamset_destroy", h)
