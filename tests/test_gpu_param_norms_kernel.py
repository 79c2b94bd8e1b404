"""Per-parameter gradient norms at the kernel level: the sum-of-squares pass keyed by segment
(zs_adamset_grad_sqnorm_segs), the per-parameter reducer over a CSR of slot ranges
(zs_sqnorm_reduce_params) and zs_param_norms.

Every expected value comes from numpy in float64 or from the restated formulas; none from the code
under test.  The bound is the project's own (DESIGN.md §4 "Error bound"): fp32 arithmetic covers
one lane's K terms of one chunk (K = 16 split master, 8 otherwise, 1 in the scalar table), all
above is double, and the result is rounded to fp32 once: (K + 2) * 2^-24 relative on a
parameter's sum of squares, half of that plus 2^-24 on its norm.

The slot rule (include/zero_amd.h): a segment's vector part has min(chunks of C, 128) slots, its
scalar part min(chunks of 256, 16), the vector part's first.
"""
import numpy as np
import pytest

from test_abi_param_norms import param_norms_ref
from test_gpu_gradnorm import CHUNK, KINDS, POISON, TERMS, _as_f64, _Dev, _grad_array, _layout, _tune

gpu_test = pytest.mark.gpu

VEC_SLOTS, SCA_SLOTS = 128, 16


def _slots(kind, segs, shifted=()):
    """The documented slot count of every segment: (vector part, scalar part)."""
    C, out = CHUNK[kind], []
    for k, (_, n, _) in enumerate(segs):
        nv = 0 if k in shifted else n & ~3
        out.append((min(-(-nv // C), VEC_SLOTS), min(-(-(n - nv) // 256), SCA_SLOTS)))
    return out


def _want(kind, g, segs):
    x = _as_f64(kind, g)
    with np.errstate(all="ignore"):
        return np.array([np.sum(x[o:o + n] ** 2) if has_g else 0.0 for o, n, has_g in segs])


def _all_grads(segs):
    return [(o, n, True) for o, n, _ in segs]


class _Segs:
    """The segmented pass of ``d`` (a ``_Dev``) and both reducers; by default one parameter per
    segment.  ``csr``: (row_ptr, slot_lo, slot_n) of another parameter -> slot-range map."""

    def __init__(self, d, csr=None):
        import torch

        self.d = d
        self.off = d.aset.sqnorm_seg_offsets
        self.n = int(self.off[-1])
        if csr is None:
            live = np.flatnonzero(np.diff(self.off) > 0)
            row_ptr = np.concatenate([[0], np.cumsum(np.diff(self.off) > 0)])
            csr = (row_ptr, self.off[:-1][live], np.diff(self.off)[live])
        self.np_ = len(csr[0]) - 1
        self.csr = [torch.from_numpy(np.asarray(a, np.int64).copy()).to(d.gpu) for a in csr]
        self.partials = torch.zeros(self.n + 8, dtype=torch.float64, device=d.gpu)
        self.out = torch.zeros(self.np_ + 1, device=d.gpu)
        self.norms = torch.zeros(self.np_, device=d.gpu)

    def run(self, div=1.0):
        """(partials as uint64 bits, per-parameter sums, the global sum, the norms), fp32."""
        import torch

        from zero_amd.kernels import param_norms, sqnorm_reduce, sqnorm_reduce_params

        d = self.d
        self.partials.fill_(-1.0)
        self.out.fill_(-1.0)
        d.aset.grad_sqnorm_segs(self.partials, d.stream)
        sqnorm_reduce_params(self.partials, *self.csr, self.np_, self.out, d.stream)
        sqnorm_reduce(self.partials, self.n, self.out[self.np_:], d.stream)
        param_norms(self.out, self.np_, div, self.norms, d.stream)
        torch.cuda.synchronize()
        part = self.partials.cpu().numpy()
        assert (part[self.n:] == -1.0).all(), "a partial was written past the set's slot count"
        out = self.out.cpu().numpy()
        return (part[:self.n].view(np.uint64).copy(), out[:self.np_].copy(), out[self.np_],
                self.norms.cpu().numpy())


def _check(kind, got, want, norms=None, div=1.0, what=""):
    bound = (TERMS[kind] + 2) * 2.0 ** -24
    worst = worst_n = 0.0
    for i, (a, w) in enumerate(zip(got, want)):
        if w == 0.0:
            assert a == 0.0 and not np.signbit(a), (what, i, a)
            continue
        assert np.isfinite(a), f"{what} entry {i}: the pass read outside a segment (or overflowed)"
        worst = max(worst, abs(float(a) - w) / w)
        if norms is not None:
            wn = np.sqrt(w) / div
            worst_n = max(worst_n, abs(float(norms[i]) - wn) / wn)
    print(f"{kind} {what}: worst rel {worst:.3e} (bound {bound:.3e}), norm {worst_n:.3e} "
          f"(bound {bound / 2 + 2.0 ** -24:.3e})")
    assert worst <= bound
    assert worst_n <= bound / 2 + 2.0 ** -24


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
def test_small_mixed_layout(gpu, kind):
    """Every segment against float64; the segment whose gradient set_grads took away is exactly
    +0.0 although POISON lies where its gradient was; slot offsets follow the documented rule;
    the global sum is the sum of all segments; the norms are the restated formula's bits."""
    C = CHUNK[kind]
    lengths = [1, 3, 4, 255, 1024, C - 4, C, C + 4, 3 * C + 1028]
    segs = _layout(lengths, no_grad=(6,), shifted=(4,))
    g = _grad_array(kind, segs, np.random.default_rng(21))
    o6, n6, _ = segs[6]
    g[o6:o6 + n6] = POISON if kind == "f32" else 0x7149  # bf16 bits of about 1e30
    d = _Dev(gpu, kind, _all_grads(segs))
    d.upload(g)
    d.aset.set_grads(np.array([_Dev.gptr(d.G, o) if has_g else 0 for o, _, has_g in segs],
                              np.uint64), d.stream)
    s = _Segs(d)
    want_off = np.concatenate([[0], np.cumsum([a + b for a, b in _slots(kind, segs, shifted=(4,))])])
    assert np.array_equal(s.off, want_off), (s.off, want_off)
    part, out, total, norms = s.run(div=3.0)
    want = _want(kind, g, segs)
    _check(kind, out, want, norms, 3.0, "mixed")
    assert out[6].view(np.uint32) == 0 and norms[6].view(np.uint32) == 0
    assert (part[s.off[6]:s.off[7]] == 0).all()  # +0.0 in every slot of the segment
    assert np.array_equal(norms.view(np.uint32), param_norms_ref(out, 3.0).view(np.uint32))
    _check(kind, [total], [want.sum()], what="mixed, global")


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
def test_workgroup_strides_over_a_segments_chunks(gpu, kind):
    """Segments with more chunks than slots: every workgroup of the vector part goes round at least
    twice (2 * 128 + 3 chunks, the last one partial, plus a tail), those of the shifted segment's
    scalar part too (2 * 16 + 2 chunks of 256)."""
    C = CHUNK[kind]
    lengths = [(2 * VEC_SLOTS + 2) * C + 4 * 11 + 3, 2 * SCA_SLOTS * 256 + 300]
    segs = _layout(lengths, shifted=(1,))
    g = _grad_array(kind, segs, np.random.default_rng(22))
    d = _Dev(gpu, kind, segs)
    d.upload(g)
    s = _Segs(d)
    assert list(np.diff(s.off)) == [VEC_SLOTS + 1, SCA_SLOTS]
    _, out, total, norms = s.run()
    want = _want(kind, g, segs)
    _check(kind, out, want, norms, 1.0, "strided")
    _check(kind, [total], [want.sum()], what="strided, global")


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
def test_a_segment_does_not_depend_on_its_neighbours(gpu, kind):
    """The same segment (vector part, partial chunk, tail) between two others and alone: the same
    slot count, the same bits in every slot and in its sum."""
    C = CHUNK[kind]
    n = 3 * C + 1028 + 3
    rng = np.random.default_rng(23)
    both = []
    for lengths, k in (([C + 12, n, 700], 1), ([n], 0)):
        segs = _layout(lengths, shifted=(2,) if len(lengths) > 1 else ())
        g = _grad_array(kind, segs, rng)
        o = segs[k][0]
        mid = _grad_array(kind, [(0, n, True)], np.random.default_rng(24))[:n]
        g[o:o + n] = mid
        d = _Dev(gpu, kind, segs)
        d.upload(g)
        s = _Segs(d)
        part, out, _, _ = s.run()
        both.append((part[s.off[k]:s.off[k + 1]], out[k]))
        _check(kind, [out[k]], [_want(kind, g, [segs[k]])[0]], what=f"{len(lengths)} segment(s)")
    assert np.array_equal(both[0][0], both[1][0])
    assert both[0][1].view(np.uint32) == both[1][1].view(np.uint32)


@gpu_test
@pytest.mark.parametrize("kind", ["split", "f32"])
def test_bits_are_the_same_on_every_run(gpu, kind):
    """Identical bits of every partial and every output from run to run, under either cache
    policy of the loads and under another grid of the update."""
    C = CHUNK[kind]
    segs = _layout([1, 255, C + 4, (VEC_SLOTS + 5) * C + 1028 + 2, 5000], shifted=(4,))
    g = _grad_array(kind, segs, np.random.default_rng(25))
    d = _Dev(gpu, kind, segs)
    d.upload(g)
    s = _Segs(d)
    bits = lambda r: (r[0], r[1].view(np.uint32), r[2].view(np.uint32), r[3].view(np.uint32))  # noqa: E731
    first = bits(s.run())
    again = bits(s.run())
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    for key, value, back in ((b"sqnorm_nt", 0, 1), (b"adam_wg_per_cu", 7, 0)):
        _tune(key, value)
        try:
            other = bits(s.run())
        finally:
            _tune(key, back)
        assert all(np.array_equal(a, b) for a, b in zip(first, other)), key


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["nan_and_inf", "square_overflows"])
def test_non_finite_entries_stay_in_their_segment(gpu, kind, case):
    """A NaN in one segment and an inf in another — or one value whose square is beyond fp32 —
    make exactly those entries non-finite; every other entry is finite and in bound; the global
    sum is non-finite."""
    C = CHUNK[kind]
    segs = _layout([3, 255, C + 4, 2 * C + 1028, 700, C], shifted=(4,))
    g = _grad_array(kind, segs, np.random.default_rng(26))
    f32 = kind == "f32"
    if case == "nan_and_inf":
        g[segs[2][0] + C + 1] = np.nan if f32 else 0x7FC0
        g[segs[4][0] + 300] = np.inf if f32 else 0x7F80
        bad = {2, 4}
    else:
        g[segs[3][0] + 2 * C + 5] = 1e30 if f32 else 0x7149  # finite; its square is not
        bad = {3}
    d = _Dev(gpu, kind, segs)
    d.upload(g)
    _, out, total, norms = _Segs(d).run()
    want = _want(kind, g, segs)
    for i in range(len(segs)):
        assert np.isfinite(out[i]) == (i not in bad), (i, out[i])
        assert np.isfinite(norms[i]) == (i not in bad), (i, norms[i])
    if case == "nan_and_inf":
        assert np.isnan(out[2]) and np.isposinf(out[4])
    else:
        assert np.isposinf(out[3])
    keep = [i for i in range(len(segs)) if i not in bad]
    _check(kind, out[keep], want[keep], norms[keep], 1.0, case)
    assert not np.isfinite(total)


@gpu_test
@pytest.mark.parametrize("kind", KINDS)
def test_a_parameter_cut_across_ranges_and_one_without_any(gpu, kind):
    """Parameter 0 owns the slots of segments 0 and 2 (two disjoint ranges, as when a parameter is
    cut across two sets), parameter 1 owns nothing, parameter 2 owns segment 1."""
    C = CHUNK[kind]
    segs = _layout([2 * C + 4 * 9, 777, C + 1028 + 1], shifted=(1,))
    g = _grad_array(kind, segs, np.random.default_rng(27))
    d = _Dev(gpu, kind, segs)
    d.upload(g)
    off = d.aset.sqnorm_seg_offsets
    n = np.diff(off)
    s = _Segs(d, csr=([0, 2, 2, 3], [off[0], off[2], off[1]], [n[0], n[2], n[1]]))
    _, out, total, norms = s.run(div=2.0)
    w = _want(kind, g, segs)
    _check(kind, out, [w[0] + w[2], 0.0, w[1]], norms, 2.0, "cut")
    assert out[1].view(np.uint32) == 0 and norms[1].view(np.uint32) == 0
    _check(kind, [total], [w.sum()], what="cut, global")
