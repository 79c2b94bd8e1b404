"""The row-scaled fp8 (OCP E4M3) quantise / dequantise kernels where they can go wrong unnoticed:
every rounding tie and E4M3 subnormal, all 256 codes under awkward scales, degenerate rows (tiny
amax, NaN, Inf), waves that walk several rows of several matrices under every compiled variant,
and the grid-stride loops at the default grid.

Every comparison is bit for bit against oracle/fp8_oracle.py (pure numpy, float64 except where the
kernel's fp32 step is the definition; pinned to torch's float8_e4m3fn by tests/test_fp8_oracle.py);
the only licence is that a NaN need only be a NaN.  Every output buffer is pre-filled with a
sentinel and checked whole, the slack behind its last row included."""

import numpy as np
import pytest
import torch

from oracle import fp8_oracle as fo
from test_fp8_oracle import bf16_values_upto_448, midpoints

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
Q_SENT, SC_SENT, Y_SENT, SLACK = 0xA5, np.float32(-12345.0), 7.0, 64


def _st():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *a):
    from zero_amd import _lib

    _lib.call(name, *a)


def _zs(dtype):
    from zero_amd.comm import zs_dtype

    return zs_dtype(dtype)


def as_input(x, dtype):
    """(CPU tensor of dtype, the float32 values it holds) of a float32 array; bf16 by the oracle's
    own RNE on the bits, so a NaN keeps its sign."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == F32:
        return torch.from_numpy(x.copy()), x
    bits = fo.f32_to_bf16_bits(x)
    return torch.from_numpy(bits.view(np.int16).copy()).view(BF16), fo.bf16_bits_to_f32(bits)


def out_bits(t):
    """uint32 / uint16 bit patterns of a float32 / bf16 tensor."""
    t = t.cpu().contiguous()
    return (t.view(torch.int32).numpy().view(np.uint32) if t.dtype == F32
            else t.view(torch.int16).numpy().view(np.uint16))


def bits_values(b):
    return fo.bf16_bits_to_f32(b) if b.dtype == np.uint16 else b.view(np.float32)


def want_deq(q, sc, dtype):
    y = fo.dequantize_rows(q, sc, "float32" if dtype == F32 else "bfloat16")
    return y.view(np.uint32) if dtype == F32 else y


def assert_same_bits(got, want, what=""):
    """Bit equality; where the oracle has a NaN, any NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = np.isnan(bits_values(want))
    assert np.isnan(bits_values(got))[nan].all(), f"{what}: a NaN came back as a number"
    bad = np.flatnonzero((got != want).ravel() & ~nan.ravel())
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: got "
                           f"{got.ravel()[bad[:5]]} want {want.ravel()[bad[:5]]}")


def assert_q(q, sc, q_want, sc_want, what=""):
    bad = np.flatnonzero(sc.view(np.uint32) != sc_want.view(np.uint32))
    assert bad.size == 0, f"{what}: scales of rows {bad[:5]}: got {sc[bad[:5]]} want {sc_want[bad[:5]]}"
    bad = np.argwhere(q != q_want)
    assert bad.size == 0, (f"{what}: {len(bad)} codes differ, first at {bad[:5].tolist()}: got "
                           f"{[hex(q[tuple(b)]) for b in bad[:5]]} want {[hex(q_want[tuple(b)]) for b in bad[:5]]}")


def quant_rows(gpu, xt):
    """zs_fp8_quantize_rows of a 2-D CPU tensor -> (q [rows, L], scales [rows]) numpy."""
    rows, L = xt.shape
    d = xt.to(gpu)
    q = torch.full((rows * L + SLACK,), Q_SENT, dtype=torch.uint8, device=gpu)
    sc = torch.full((rows + SLACK,), float(SC_SENT), dtype=F32, device=gpu)
    _call("zs_fp8_quantize_rows", d.data_ptr(), _zs(xt.dtype), q.data_ptr(), sc.data_ptr(), rows, L, _st())
    torch.cuda.synchronize()
    qh, sh = q.cpu().numpy(), sc.cpu().numpy()
    assert (qh[rows * L:] == Q_SENT).all() and (sh[rows:] == SC_SENT).all(), "a store behind the last row"
    return qh[:rows * L].reshape(rows, L), sh[:rows]


def quant_rowset(gpu, mats):
    """zs_fp8_quantize_rowset over [(2-D CPU tensor, cs >= rows)] -> [(q [cs, L], scales [cs])]."""
    dtype = mats[0][0].dtype
    n = len(mats)
    devs = [xt.to(gpu) for xt, _ in mats]
    cs = np.array([c for _, c in mats], np.int64)
    rows = np.array([xt.shape[0] for xt, _ in mats], np.int64)
    rl = np.array([xt.shape[1] for xt, _ in mats], np.int64)
    q_off = np.concatenate([[0], np.cumsum(cs * rl)]).astype(np.int64)
    sc_off = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    q = torch.full((int(q_off[-1]) + SLACK,), Q_SENT, dtype=torch.uint8, device=gpu)
    sc = torch.full((int(sc_off[-1]) + SLACK,), float(SC_SENT), dtype=F32, device=gpu)
    src = np.array([d.data_ptr() for d in devs], np.uint64)
    qp = np.uint64(q.data_ptr()) + q_off[:-1].astype(np.uint64)
    sp = np.uint64(sc.data_ptr()) + (4 * sc_off[:-1]).astype(np.uint64)
    _call("zs_fp8_quantize_rowset", n, src.ctypes.data, qp.ctypes.data, sp.ctypes.data,
          rows.ctypes.data, cs.ctypes.data, rl.ctypes.data, _zs(dtype), _st())
    torch.cuda.synchronize()
    qh, sh = q.cpu().numpy(), sc.cpu().numpy()
    assert (qh[q_off[-1]:] == Q_SENT).all() and (sh[sc_off[-1]:] == SC_SENT).all(), "a store behind the last row"
    return [(qh[q_off[m]:q_off[m + 1]].reshape(cs[m], rl[m]), sh[sc_off[m]:sc_off[m + 1]]) for m in range(n)]


def dequant_rows(gpu, q, sc, dtype):
    """zs_fp8_dequantize_rows of numpy (q [rows, L], scales) -> bit patterns [rows, L]."""
    rows, L = q.shape
    dq = torch.from_numpy(np.ascontiguousarray(q)).to(gpu)
    ds = torch.from_numpy(np.ascontiguousarray(sc, np.float32)).to(gpu)
    y = torch.full((rows * L + SLACK,), Y_SENT, dtype=dtype, device=gpu)
    _call("zs_fp8_dequantize_rows", dq.data_ptr(), ds.data_ptr(), y.data_ptr(), _zs(dtype), rows, L, _st())
    torch.cuda.synchronize()
    b = out_bits(y)
    assert (b[rows * L:] == b[-1]).all() and bits_values(b[-1:])[0] == Y_SENT, "a store behind the last row"
    return b[:rows * L].reshape(rows, L)


def dequant_gathered(gpu, ws, shapes, qr, sr, dtype):
    """zs_fp8_dequantize_gathered of the rank-major buffers (qr [ws * qtot] bytes, sr [ws * sctot])
    of the matrices shapes = [(cs, L)] -> [bit patterns [ws * cs, L]]; the outputs lie back to
    back in one sentinel-filled buffer."""
    n = len(shapes)
    cs = np.array([c for c, _ in shapes], np.int64)
    rl = np.array([r for _, r in shapes], np.int64)
    q_off = np.concatenate([[0], np.cumsum(cs * rl)]).astype(np.int64)
    sc_off = np.concatenate([[0], np.cumsum(cs)]).astype(np.int64)
    qtot, sctot = int(q_off[-1]), int(sc_off[-1])
    assert qr.size == ws * qtot and sr.size == ws * sctot
    y_off = np.concatenate([[0], np.cumsum(ws * cs * rl)]).astype(np.int64)
    dq = torch.from_numpy(np.ascontiguousarray(qr)).to(gpu)
    ds = torch.from_numpy(np.ascontiguousarray(sr, np.float32)).to(gpu)
    y = torch.full((int(y_off[-1]) + SLACK,), Y_SENT, dtype=dtype, device=gpu)
    dst = np.uint64(y.data_ptr()) + (y.element_size() * y_off[:-1]).astype(np.uint64)
    qo, so = q_off[:-1].copy(), sc_off[:-1].copy()
    _call("zs_fp8_dequantize_gathered", n, dq.data_ptr(), ds.data_ptr(), ws, qtot, sctot,
          qo.ctypes.data, so.ctypes.data, cs.ctypes.data, rl.ctypes.data, dst.ctypes.data, _zs(dtype), _st())
    torch.cuda.synchronize()
    b = out_bits(y)
    assert (b[y_off[-1]:] == b[-1]).all() and bits_values(b[-1:])[0] == Y_SENT, "a store behind the last row"
    return [b[y_off[m]:y_off[m + 1]].reshape(ws * cs[m], rl[m]) for m in range(n)]


def gathered_rows(ws, shapes, qr, sr):
    """The full matrices (q [ws * cs, L], scales [ws * cs]) that the rank-major buffers hold: full
    row R of matrix m is rank R // cs's local row R % cs."""
    cs = [c for c, _ in shapes]
    qtot, sctot = sum(c * r for c, r in shapes), sum(cs)
    out, qo, so = [], 0, 0
    for c, r in shapes:
        q = np.concatenate([qr[k * qtot + qo:k * qtot + qo + c * r] for k in range(ws)]).reshape(ws * c, r)
        s = np.concatenate([sr[k * sctot + so:k * sctot + so + c] for k in range(ws)])
        out.append((q, s))
        qo, so = qo + c * r, so + c
    return out


def nreg(L, dtype):
    """The register class zs_fp8_quantize_rows / _rowset pick for a row length (0: streamed)."""
    chunks = -(-L // (64 * (4 if dtype == F32 else 8)))
    return 8 if chunks <= 8 else 16 if chunks <= 16 else 32 if chunks <= 32 else 0


def tune(**kw):
    for k, v in kw.items():
        _call("zs_tune", k.encode(), int(v), None)


DQ_DEFAULT = dict(dq_unroll=4, dq_nt_store=1, dq_wg_per_cu=0)


def cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


# ------------------------------------------------------------------------------------------------
# 1. exhaustive rounding, quantise
# ------------------------------------------------------------------------------------------------
def _layout(vals, L, top):
    """Rows of L elements: +top, -top, then L - 2 of the values (zero-padded at the end)."""
    per = L - 2
    rows = -(-vals.size // per)
    body = np.zeros(rows * per, np.float32)
    body[:vals.size] = vals
    m = np.empty((rows, L), np.float32)
    m[:, 0], m[:, 1] = top, -top
    m[:, 2:] = body.reshape(rows, per)
    return m


@pytest.mark.parametrize("exp", [0, -20, 20])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_quantize_every_tie_and_subnormal(gpu, dtype, exp):
    """Every bf16 value of |x| <= 448 (both signs; every E4M3 tie and subnormal is among them), for
    fp32 also every tie +- 1 fp32 ulp, in rows that hold +-448: inv = 1 and scale = 1 exactly.
    Times 2^exp: inv = 2^-exp, scale = 2^exp, the same codes.  Through the streamed path (one long
    row), the register classes 8 / 16 / 32, the block-per-row fallback and the rowset kernel."""
    vals = bf16_values_upto_448()
    if dtype == F32:
        mid = midpoints()
        nb = np.concatenate([np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))])
        vals = np.concatenate([vals, nb, -nb])
    k = np.float32(2.0 ** exp)
    E = 4 if dtype == F32 else 8
    long_len = -(-(vals.size + 2) // 8) * 8
    lens = {0: long_len, 8: 1000, 16: 64 * E * 8 + 8, 32: 64 * E * 16 + 8}
    assert long_len > 16384 and all(nreg(L, dtype) == c for c, L in lens.items())
    lens["fallback"] = 1001  # no multiple of 8: block per row, scalar accesses
    mats = {}
    for c, L in lens.items():
        xt, xv = as_input(_layout(vals * k, L, np.float32(448.0) * k), dtype)
        q_want, sc_want = fo.quantize_rows(xv)
        # the inputs do what they are meant to: scale 2^exp in every row, codes independent of exp
        # (a value that the scaling rounds lies below 2^-100 of its row's amax: code 0 either way)
        assert (sc_want == k).all()
        assert np.array_equal(q_want, fo.quantize_rows(as_input(_layout(vals, L, 448.0), dtype)[1])[0])
        mats[c] = (xt, q_want, sc_want)
        q, sc = quant_rows(gpu, xt)
        assert_q(q, sc, q_want, sc_want, f"rows, class {c}")
    keys = [0, 8, 16, 32]
    got = quant_rowset(gpu, [(mats[c][0], mats[c][0].shape[0] + (1 if c == 8 else 0)) for c in keys])
    for c, (q, sc) in zip(keys, got):
        r = mats[c][0].shape[0]
        assert_q(q[:r], sc[:r], mats[c][1], mats[c][2], f"rowset, class {c}")
        assert not q[r:].any() and (sc[r:] == 1).all()


# ------------------------------------------------------------------------------------------------
# 2. exhaustive dequantise
# ------------------------------------------------------------------------------------------------
DQ_SCALES = np.array([1.0, 2.0 ** -20, np.float32(0.1), np.float32(3e-40), 2.0 ** 100], np.float32)


def _all_codes(L):
    """Two rows per scale, each a rotation of the 256 codes cut to L: with L = 251 the two rows of
    a scale miss different codes, so every code meets every scale."""
    sc = np.repeat(DQ_SCALES, 2)
    q = np.stack([np.roll(np.arange(256, dtype=np.uint8), -37 * i)[:L] for i in range(sc.size)])
    for s in range(DQ_SCALES.size):
        assert np.unique(q[2 * s:2 * s + 2]).size == 256
    return q, sc


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_dequantize_every_code(gpu, dtype):
    """All 256 codes under the scales 1, 2^-20, 0.1 (no power of two), a denormal (the library is
    built with denormals on) and 2^100, through the vector path (256), the scalar fallback (251)
    and the gathered kernel at ws = 2: code -> fp32 exactly, one fp32 rounding of the product, RNE
    to bf16; the two NaN codes come back NaN."""
    assert 0 < DQ_SCALES[3] < np.finfo(np.float32).tiny
    for L in (256, 251):
        q, sc = _all_codes(L)
        want = want_deq(q, sc, dtype)
        got = dequant_rows(gpu, q, sc, dtype)
        assert_same_bits(got, want, f"rows, L {L}")
        nan_code = (q & 0x7F) == 0x7F
        assert nan_code.sum() >= sc.size and np.array_equal(np.isnan(bits_values(got)), nan_code)
    q, sc = _all_codes(256)
    (got,) = dequant_gathered(gpu, 2, [(q.shape[0] // 2, 256)], q.reshape(-1), sc, dtype)
    assert_same_bits(got, want_deq(q, sc, dtype), "gathered, ws 2")


# ------------------------------------------------------------------------------------------------
# 3. degenerate rows
# ------------------------------------------------------------------------------------------------
BF16_MAX = np.array([0x7F7F0000], np.uint32).view(np.float32)[0]
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]


def _degenerate(L, seed):
    """(x [19, L] float32, {kind: row}): the degenerate rows, an ordinary row on either side of each."""
    rng = np.random.default_rng(seed)
    f = np.float32

    def ordinary():
        return (rng.standard_normal(L) * 10.0 ** rng.integers(-3, 3)).astype(f)

    def unit(lim=1.0):
        return rng.uniform(-lim, lim, L).astype(f)

    kinds = {}
    rows = [ordinary()]

    def add(kind, r):
        kinds[kind] = len(rows)
        rows.extend([r.astype(f), ordinary()])

    add("zero", np.zeros(L))
    r = np.where(rng.random(L) < 0.3, 0, np.where(rng.random(L) < 0.5, -1, 1) * f(1e-37)).astype(f)
    r[:4] = [1e-37, 0.0, -1e-37, -0.0]
    add("tiny", r)
    r = unit() * f(2.0 ** -116)
    r[L // 2], r[1] = 2.0 ** -116, 0.0
    add("floor", r)  # amax exactly at the floor: today's formula, today's bits
    r = unit() * f(1e-36)
    r[1], r[5] = 1e-36, 0.0
    add("1e-36", r)
    r = ordinary()
    r[L // 3] = np.nan
    add("one_nan", r)
    r = np.full(L, np.nan, f)
    r[1::2] = NEG_NAN
    add("all_nan", r)
    r = ordinary()
    r[2] = np.inf
    add("inf", r)
    r = ordinary()
    r[4], r[7], r[9] = -np.inf, np.nan, NEG_NAN
    add("neg_inf_nan", r)
    r = unit(0.9) * BF16_MAX
    r[3] = BF16_MAX
    add("bf16_max", r)
    return np.stack(rows), kinds


def _check_degenerate(xv, kinds, q, sc, deq_bits, q_alone, sc_alone, what):
    """The contract, row by row (oracle equality is asserted by the caller)."""
    y = bits_values(deq_bits)
    nan_in = np.isnan(xv)
    assert (q[nan_in] == fo.ROW_NAN_CODE).all(), f"{what}: a NaN element is not stored as the NaN code"
    assert np.isnan(y)[nan_in].all(), f"{what}: a NaN element dequantises to a number"
    for kind in ("tiny", "floor", "1e-36"):
        r = kinds[kind]
        assert np.isfinite(y[r]).all() and sc[r] >= np.finfo(np.float32).tiny, (what, kind)
        assert ((q[r] & 0x7F) == 0)[xv[r] == 0].all(), f"{what}: a zero of the {kind} row is not code 0"
        assert np.max(np.abs(y[r].astype(np.float64) - xv[r])) <= max(2.0 ** -116, np.max(np.abs(xv[r]))) / 28 * 1.01
    for kind in ("tiny", "1e-36"):
        assert sc[kinds[kind]] == np.float32(2.0 ** -116) / np.float32(448)
    r = kinds["one_nan"]
    assert np.isfinite(y[r][~nan_in[r]]).all() and np.isfinite(sc[r])
    assert sc[kinds["all_nan"]] == 1 and sc[kinds["zero"]] == 1 and not q[kinds["zero"]].any()
    for kind in ("inf", "neg_inf_nan"):
        r = kinds[kind]
        assert sc[r] == np.inf and not np.isfinite(y[r]).any(), f"{what}: {kind} row"
    assert np.isfinite(y[kinds["bf16_max"]]).all()
    # the rows beside a degenerate row: the bits they get when quantised on their own
    ordinary = np.arange(0, xv.shape[0], 2)
    assert np.isfinite(y[ordinary]).all()
    assert_q(q[ordinary], sc[ordinary], q_alone, sc_alone, f"{what}: ordinary rows beside degenerate ones")


@pytest.mark.parametrize("path", ["resident", "streamed", "fallback", "rowset"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_degenerate_rows(gpu, dtype, path):
    """DESIGN.md §4 "fp8 rows: the contract" on every quantise path: rows with amax below 2^-116
    are scaled as though amax were 2^-116 (zeros stay code 0, nothing becomes NaN); a NaN element
    is the NaN code 0xFF and comes back NaN, the rest of its row untouched; a row that holds an Inf has
    scale +inf and no finite element; the rows around them are untouched."""
    lens = {"resident": [64], "streamed": [16392], "fallback": [37], "rowset": [64, 16392]}[path]
    assert [nreg(L, dtype) for L in lens] == {"resident": [8], "streamed": [0], "fallback": [8],
                                              "rowset": [8, 0]}[path]
    ins = []
    for L in lens:
        x, kinds = _degenerate(L, L)
        xt, xv = as_input(x, dtype)
        at, _ = as_input(x[::2], dtype)
        ins.append((xt, xv, kinds, at))
    if path == "rowset":
        got = quant_rowset(gpu, [(xt, xt.shape[0] + 2 * i) for i, (xt, _, _, _) in enumerate(ins)])
        alone = quant_rowset(gpu, [(at, at.shape[0]) for _, _, _, at in ins])
    else:
        got = [quant_rows(gpu, xt) for xt, _, _, _ in ins]
        alone = [quant_rows(gpu, at) for _, _, _, at in ins]
    for (xt, xv, kinds, _), (q, sc), (qa, sa) in zip(ins, got, alone):
        rows, L = xv.shape
        what = f"{path}, L {L}"
        q_want, sc_want = fo.quantize_rows(xv)
        print(what, "scales got", sc[1::2], "want", sc_want[1::2])
        assert not q[rows:].any() and (sc[rows:] == 1).all()  # (rowset padding)
        q, sc = q[:rows], sc[:rows]
        deq = dequant_rows(gpu, q, sc, dtype)
        _check_degenerate(xv, kinds, q, sc, deq, qa, sa, what)
        assert_q(q, sc, q_want, sc_want, what)
        assert_same_bits(deq, want_deq(q_want, sc_want, dtype), what)


# ------------------------------------------------------------------------------------------------
# 4. waves that walk several rows of several matrices, every compiled variant
# ------------------------------------------------------------------------------------------------
WALK_WS = 3
WALK_SHAPES = [(700, 24), (0, 64), (350, 2056), (3, 16392), (500, 8)]  # (cs, row_len)
WALK_SETTINGS = [None, (4, 1, 1), (8, 1, 1), (16, 1, 1), (4, 0, 1), (8, 0, 0), (16, 1, 0)]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_gathered_waves_walk_rows_every_variant(gpu, dtype):
    """zs_fp8_dequantize_gathered at ws = 3 with at most one workgroup per CU, so every wave takes
    rows g, g + nwaves, ... (at least three each): the next row's loads — of another matrix with
    another row length, across an empty matrix — are issued before the current row's stores and
    handed over.  U = 4 / 8 / 16 accesses per lane, plain and non-temporal stores, and the default
    launch all give the oracle's bits, hence each other's."""
    rng = np.random.default_rng(11)
    ws, shapes = WALK_WS, WALK_SHAPES
    total = ws * sum(c for c, _ in shapes)
    for s in WALK_SETTINGS:
        if s is not None and s[2] > 0:
            nwaves = 4 * cus(gpu) * s[2]
            assert total >= 3 * nwaves, (total, nwaves)
    qr = rng.integers(0, 256, ws * sum(c * r for c, r in shapes), dtype=np.uint8)
    sr = (rng.uniform(0.5, 2.0, total) * 10.0 ** rng.integers(-6, 6, total)).astype(np.float32)
    want = [want_deq(q, s, dtype) for q, s in gathered_rows(ws, shapes, qr, sr)]
    first = None
    try:
        for s in WALK_SETTINGS:
            tune(**(DQ_DEFAULT if s is None else dict(zip(DQ_DEFAULT, s))))
            got = dequant_gathered(gpu, ws, shapes, qr, sr, dtype)
            for m, (g, w) in enumerate(zip(got, want)):
                assert_same_bits(g, w, f"setting {s}, matrix {m}")
            if first is None:
                first = got
            for m, (g, f) in enumerate(zip(got, first)):  # NaN payloads included
                assert np.array_equal(g, f), f"setting {s} differs from the default, matrix {m}"
    finally:
        tune(**DQ_DEFAULT)


# ------------------------------------------------------------------------------------------------
# 5. grid-stride loops at the default grid
# ------------------------------------------------------------------------------------------------
def _rows_data(rows, L, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, L)).astype(np.float32) * (10.0 ** rng.integers(-4, 5, (rows, 1))).astype(np.float32)
    x[::97] = 0
    return x


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_rows_kernels_stride_past_the_grid(gpu, dtype):
    """More rows than the wave-per-row kernels have waves (4 per workgroup, 128 workgroups per CU):
    the quantise loop and the dequantise walk both go round again."""
    rows, L = 4 * 128 * cus(gpu) + 1037, 8
    assert rows > 4 * min((rows + 3) // 4, 128 * cus(gpu))
    xt, xv = as_input(_rows_data(rows, L, 1), dtype)
    q_want, sc_want = fo.quantize_rows(xv)
    # the product is not clamped before the conversion: rows whose largest element lands one fp32
    # ulp above 448 (it must still be code 0x7E) are among these
    amax, inv, _ = fo.row_scales(xv)
    assert ((amax * inv).astype(np.float32) > 448).sum() > 1000
    q, sc = quant_rows(gpu, xt)
    assert_q(q, sc, q_want, sc_want, "quantise")
    assert_same_bits(dequant_rows(gpu, q_want, sc_want, dtype), want_deq(q_want, sc_want, dtype), "dequantise")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_block_per_row_fallback_strides_past_the_grid(gpu, dtype):
    rows, L = 128 * cus(gpu) + 517, 5
    assert rows > min(rows, 128 * cus(gpu))
    xt, xv = as_input(_rows_data(rows, L, 2), dtype)
    q, sc = quant_rows(gpu, xt)
    assert_q(q, sc, *fo.quantize_rows(xv), "quantise, block per row")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_rowset_strides_past_the_grid_with_padding_rows(gpu, dtype):
    """Three matrices of one register class (one launch) with more rows than the launch has waves;
    the first and the last have padding rows (rows < cs), the last one's on a later stride:
    q = 0, scale = 1 there."""
    nwaves = 4 * 128 * cus(gpu)
    shapes = [(nwaves // 2, nwaves // 2 - 300, 8), (nwaves // 2, nwaves // 2, 16), (1037, 937, 8)]  # cs, rows, L
    total = sum(c for c, _, _ in shapes)
    assert total > 4 * min((total + 3) // 4, 128 * cus(gpu)) == nwaves
    assert total - shapes[2][0] + shapes[2][1] >= nwaves  # the last matrix's padding rows: second stride
    assert len({nreg(L, dtype) for _, _, L in shapes}) == 1
    ins = [as_input(_rows_data(r, L, 3 + i), dtype) for i, (_, r, L) in enumerate(shapes)]
    got = quant_rowset(gpu, [(xt, c) for (xt, _), (c, _, _) in zip(ins, shapes)])
    for m, ((q, sc), (_, xv), (c, r, L)) in enumerate(zip(got, ins, shapes)):
        assert_q(q[:r], sc[:r], *fo.quantize_rows(xv), f"matrix {m}")
        assert q[r:].shape == (c - r, L) and not q[r:].any(), f"matrix {m}: padding rows' q"
        assert np.array_equal(sc[r:], np.ones(c - r, np.float32)), f"matrix {m}: padding rows' scale"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_scalar_dequantize_strides_past_the_grid(gpu, dtype):
    L = 5
    rows = 128 * cus(gpu) * 256 // L + 211
    n = rows * L
    assert n > 256 * min((n + 255) // 256, 128 * cus(gpu))
    rng = np.random.default_rng(4)
    q = rng.integers(0, 256, (rows, L), dtype=np.uint8)
    sc = (rng.uniform(0.5, 2.0, rows) * 10.0 ** rng.integers(-6, 6, rows)).astype(np.float32)
    assert_same_bits(dequant_rows(gpu, q, sc, dtype), want_deq(q, sc, dtype), "scalar dequantise")
