"""The vector Adam kernel's two chunk paths: full chunks through the loads-first body, partial
chunks (and everything under ``zs_tune("adam_loads_first", 0)``) through the predicated body.

Every case runs 3 steps with the switch at 0 and at 1 on the same inputs and compares every array
the kernel writes, bit for bit, against the C oracle (computed once per case) and between the two
switch settings.  The arrays are compared whole, gaps between segments and the slack behind the
last one included, so a store outside a segment shows as well.  C below is the chunk of the
instance: 4,096 elements for the split master, 2,048 otherwise.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import zero_oracle as zo

pytestmark = pytest.mark.gpu

KINDS = ("split", "bf16", "f32")  # bf16 grad + split master / bf16 grad + fp32 master / fp32 grad
CHUNK = {"split": 4096, "bf16": 2048, "f32": 2048}
STEPS = 3
SLACK = 4096  # elements behind the last segment that nothing may touch
# every tie class of the split encoding (tests/test_gpu_kernels.py): exact ties under an even and
# an odd bf16 param (the even ones store the 0x7FFF residual), both signs, a denormal tie, values
# next to the bf16 overflow threshold
TIES = np.array([0x3C808000, 0x3C818000, 0xBC808000, 0xBC818000, 0x00008000, 0x80008000,
                 0x7F7F7FFF, 0x7F7F8000, 0x3F80FFFF, 0x00000000], np.uint32)


def _tune(key, value):
    from zero_amd import _lib

    _lib.call("zs_tune", key, int(value), None)


class _Case:
    """Host inputs of one case: a flat arena and segments (offset, n, has_grad) in it."""

    def __init__(self, kind, segs, seed, *, ams=False, carry=False, nan_at=(), hp=None):
        self.kind, self.segs, self.ams, self.carry = kind, segs, ams, carry
        self.hp = dict(hp or {})
        if carry:
            self.hp.update(grad_div=3.0, carry_mul=2.0)
        rng = np.random.default_rng(seed)
        self.N = N = max(o + n for o, n, _ in segs) + SLACK
        self.master0 = (rng.standard_normal(N) * 0.02).astype(np.float32)
        u = self.master0.view(np.uint32)
        for o, n, _ in segs:  # ties at the head of every segment and of its second chunk
            for at in (o, o + CHUNK[kind]):
                k = max(0, min(len(TIES), o + n - at))
                u[at:at + k] = TIES[:k]
        self.grads = []
        for _ in range(STEPS):
            g = (rng.standard_normal(N) * 1e-2).astype(np.float32)
            if kind != "f32":
                g = zo.f32_to_bf16_bits(g)
            for at in nan_at:
                g[at] = np.float32(np.nan) if kind == "f32" else 0x7FC0
            self.grads.append(g)

    # ---- the C oracle, segment by segment, in place on slices of the arena ----
    def reference(self):
        N, kind = self.N, self.kind
        out = {"m": np.zeros(N, np.float32), "v": np.zeros(N, np.float32)}
        if self.ams:
            out["vmax"] = np.zeros(N, np.float32)
        if self.carry:
            out["carry"] = np.zeros(N, np.float32)
        if kind == "split":
            out["hi"], out["lo"] = c_oracle.split_master(self.master0)
        else:
            out["p"] = self.master0.copy()
            if kind == "bf16":
                out["pb"] = np.zeros(N, np.uint16)
        for t in range(1, STEPS + 1):
            hp = c_oracle.hparams(step=t, amsgrad=self.ams, **self.hp)
            for o, n, has_g in self.segs:
                sl = slice(o, o + n)
                g = self.grads[t - 1][sl].copy()
                if not has_g:
                    g[:] = 0
                opt = dict(vmax=out["vmax"][sl] if self.ams else None,
                           carry=out["carry"][sl] if self.carry else None)
                if kind == "split":
                    c_oracle.adam_bf16_split(out["hi"][sl], out["lo"][sl], g, out["m"][sl],
                                             out["v"][sl], hp, **opt)
                elif kind == "bf16":
                    c_oracle.adam_bf16(out["p"][sl], out["pb"][sl], g, out["m"][sl], out["v"][sl],
                                       hp, **opt)
                else:
                    c_oracle.adam_f32(out["p"][sl], g, out["m"][sl], out["v"][sl], hp, **opt)
        return out

    # ---- the kernels ----
    def run_gpu(self, gpu, loads_first, wg_per_cu=0):
        from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT, ZS_F32
        from zero_amd.kernels import AdamSet, adam_hparams

        N, kind = self.N, self.kind
        dev = lambda a: torch.from_numpy(a.copy()).to(gpu)  # noqa: E731
        bits = lambda a: dev(a.view(np.int16))  # noqa: E731
        T = {"m": torch.zeros(N, device=gpu), "v": torch.zeros(N, device=gpu)}
        if self.ams:
            T["vmax"] = torch.zeros(N, device=gpu)
        if self.carry:
            T["carry"] = torch.zeros(N, device=gpu)
        if kind == "split":
            hi0, lo0 = c_oracle.split_master(self.master0)
            T["hi"], T["lo"] = bits(hi0), bits(lo0)
        else:
            T["p"] = dev(self.master0)
            if kind == "bf16":
                T["pb"] = torch.zeros(N, dtype=torch.int16, device=gpu)
        G = torch.zeros(N, dtype=torch.float32 if kind == "f32" else torch.int16, device=gpu)
        at = lambda name, o: T[name].data_ptr() + o * T[name].element_size() if name in T else 0  # noqa: E731
        rows = []
        for o, n, has_g in self.segs:
            g = G.data_ptr() + o * G.element_size() if has_g else 0
            if kind == "split":
                row = [g, at("hi", o), at("lo", o), at("hi", o)]
            else:
                row = [g, at("p", o), at("p", o), at("pb", o)]
            rows.append(row + [at("m", o), at("v", o), at("vmax", o), at("carry", o), n])
        g_dtype = ZS_F32 if kind == "f32" else ZS_BF16
        aset = AdamSet(np.array(rows, dtype=np.uint64), g_dtype,
                       ZS_BF16_SPLIT if kind == "split" else ZS_BF16)
        st = torch.cuda.current_stream()
        _tune(b"adam_loads_first", loads_first)
        _tune(b"adam_wg_per_cu", wg_per_cu)
        try:
            for t in range(1, STEPS + 1):
                g = self.grads[t - 1]
                G.copy_(torch.from_numpy(g if kind == "f32" else g.view(np.int16)))
                aset.run(adam_hparams(1e-3, 0.9, 0.999, 1e-8, self.hp.get("weight_decay", 0.0), t,
                                      amsgrad=self.ams,
                                      **{k: v for k, v in self.hp.items() if k != "weight_decay"}),
                         st)
            torch.cuda.synchronize()
        finally:
            _tune(b"adam_loads_first", 1)
            _tune(b"adam_wg_per_cu", 0)
        return {k: v.cpu().numpy() for k, v in T.items()}


def _as_bits(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint16)


def _check(gpu, case, wg_per_cu=0):
    want = case.reference()
    got = {lf: case.run_gpu(gpu, lf, wg_per_cu) for lf in (0, 1)}
    for name, ref in want.items():
        for lf in (0, 1):
            a, b = _as_bits(got[lf][name]), _as_bits(ref)
            bad = np.flatnonzero(a != b)
            assert bad.size == 0, (f"{name}, adam_loads_first={lf}: {bad.size} elements differ from "
                                   f"the oracle, first at {bad[:8]}")
        assert np.array_equal(_as_bits(got[0][name]), _as_bits(got[1][name])), name


def _lengths(C):
    return [4, C - 4, C, C + 4, 2 * C, 2 * C + 4, 3 * C - 4]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", range(7))
def test_boundary_lengths(gpu, kind, k):
    """One segment of n = 4, C-4, C, C+4, 2C, 2C+4, 3C-4: partial only, exactly full, full chunks
    followed by a partial one."""
    n = _lengths(CHUNK[kind])[k]
    _check(gpu, _Case(kind, [(0, n, True)], seed=100 + k))


def _mixed_table(C):
    """Two segments of many full chunks around: one shorter than a chunk, one without a gradient
    (between two that have one), one unaligned (the scalar kernel), one with a partial last chunk."""
    segs, off = [], 0
    for n, has_g, shift in ((300 * C, True, 0), (C - 8, True, 0), (3 * C + 4, False, 0),
                            (2 * C, True, 0), (C + 7, True, 1), (300 * C + 12, True, 0)):
        off = (off + 3) // 4 * 4 + shift  # 16-byte aligned, or one element off
        segs.append((off, n, has_g))
        off += n
    return segs


@pytest.mark.parametrize("kind", ["split", "f32"])
@pytest.mark.parametrize("wg_per_cu", [1, 0])
def test_mixed_table(gpu, kind, wg_per_cu):
    """The forward scan across segments of every kind in one table; with one workgroup per CU the
    grid is smaller than the chunk count, so every workgroup loops over several chunks and
    segments; then the default grid."""
    segs = _mixed_table(CHUNK[kind])
    if wg_per_cu:
        chunks = sum(n // CHUNK[kind] for _, n, _ in segs)
        assert 2 * wg_per_cu * torch.cuda.get_device_properties(gpu).multi_processor_count <= chunks
    _check(gpu, _Case(kind, segs, seed=7), wg_per_cu)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ams", [False, True])
@pytest.mark.parametrize("carry", [False, True])
def test_every_instance(gpu, kind, ams, carry):
    """Every compiled combination of gradient type, master layout, amsgrad and carry at 2C+4."""
    _check(gpu, _Case(kind, [(0, 2 * CHUNK[kind] + 4, True)], seed=11, ams=ams, carry=carry))


def scalar_table_past_the_grid(cus):
    """(segments, scalar chunks): a table whose scalar part has more than 2 * cus chunks of 256
    elements.  Two long segments one element off alignment (scalar throughout) around an aligned
    7-element one (a 3-element tail entry) and an unaligned one without a gradient."""
    segs, off, sca_chunks = [], 0, 0
    for n, has_g, shift in ((256 * cus + 300, True, 1), (7, True, 0), (300, False, 1),
                            (256 * cus + 513, True, 1)):
        off = (off + 3) // 4 * 4 + shift  # 16-byte aligned, or one element off
        segs.append((off, n, has_g))
        off += n
        sca_chunks += -(-(n if shift else n % 4) // 256)  # aligned: only the n % 4 tail is scalar
    return segs, sca_chunks


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ams", [False, True])
@pytest.mark.parametrize("carry", [False, True])
def test_scalar_table_strides_past_the_grid(gpu, kind, ams, carry):
    """Every scalar instance with one workgroup per CU over a scalar table of more than 2 * cus
    chunks: every workgroup goes round its stride loop at least twice, and its forward scan
    crosses all four entries."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    segs, sca_chunks = scalar_table_past_the_grid(cus)
    assert sca_chunks == 2 * cus + 8 and sca_chunks > 2 * cus
    _check(gpu, _Case(kind, segs, seed=31, ams=ams, carry=carry), wg_per_cu=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hp", [dict(weight_decay=1e-2), dict(maximize=True), dict(grad_div=3.0)],
                         ids=["wd", "maximize", "div3"])
def test_awkward_inputs(gpu, kind, hp):
    """Tie residuals in the master (0x7FFF), a NaN gradient element in a full chunk and one in the
    partial chunk, with weight decay, maximize and a divisor that is no power of two."""
    C = CHUNK[kind]
    _check(gpu, _Case(kind, [(0, 2 * C + 4, True)], seed=23, nan_at=(C + 5, 2 * C + 1), hp=hp))
