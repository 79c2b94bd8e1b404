"""oracle/fp8_oracle.py (the numpy statement of OCP E4M3 and of the row-scaled fp8 contract) pinned
against torch's own float8_e4m3fn conversion wherever the two are defined alike: every code, every
bf16 value of |x| <= 448, every rounding midpoint and its fp32 neighbours."""

import numpy as np
import torch

from oracle import fp8_oracle as fo


def _torch_encode(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def bf16_values_upto_448() -> np.ndarray:
    """Every bf16 bit pattern with |x| <= 448, both signs, as float32 (34,754 values)."""
    top = int(fo.f32_to_bf16_bits(np.float32([448.0]))[0])
    assert top == 0x43E0
    pos = np.arange(top + 1, dtype=np.uint16)
    return fo.bf16_bits_to_f32(np.concatenate([pos, pos | np.uint16(0x8000)]))


def midpoints() -> np.ndarray:
    """Every midpoint between neighbouring non-negative E4M3 values (126 of them), float32."""
    v = fo.e4m3_decode(np.arange(0x7F, dtype=np.uint8))
    mid = (v[:-1] + v[1:]) / 2
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)
    return mid.astype(np.float32)


def test_decode_all_codes_matches_torch():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    got = fo.e4m3_decode(codes)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert sorted(codes[np.isnan(got)]) == [0x7F, 0xFF]
    fin = ~np.isnan(got)
    assert np.array_equal(got[fin], want[fin])
    assert np.array_equal(np.signbit(got), np.signbit(want) | (codes == 0xFF))
    assert got[0x7E] == 448.0 and got[0x01] == 2.0 ** -9 and got[0x08] == 2.0 ** -6


def test_encode_all_codes_round_trip():
    codes = np.arange(256, dtype=np.uint8)
    vals = fo.e4m3_decode(codes).astype(np.float32)
    assert np.array_equal(fo.e4m3_encode(vals), codes)  # NaN codes keep their sign, -0 stays 0x80
    assert np.array_equal(_torch_encode(vals), codes)


def test_encode_every_bf16_value_matches_torch():
    x = bf16_values_upto_448()
    assert x.size == 2 * 0x43E1
    # every midpoint is itself a bf16 value, so this set already holds every tie
    assert np.isin(midpoints(), x).all()
    assert np.array_equal(fo.e4m3_encode(x), _torch_encode(x))


def test_encode_midpoints_and_neighbours_match_torch():
    mid = midpoints()
    pts = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))])
    pts = np.concatenate([pts, -pts])
    got = fo.e4m3_encode(pts)
    assert np.array_equal(got, _torch_encode(pts))
    # the ties themselves go to the even code, one ulp either side to the nearer neighbour
    n = mid.size
    lo = np.arange(n, dtype=np.uint8)
    assert np.array_equal(got[:n], np.where(lo % 2 == 0, lo, lo + 1))
    assert np.array_equal(got[n:2 * n], lo + 1) and np.array_equal(got[2 * n:3 * n], lo)


def test_encode_saturates_and_keeps_nan_sign():
    x = np.array([448.0, 449.0, 464.0, 1e30, np.inf, -500.0, -np.inf], np.float32)
    assert fo.e4m3_encode(x).tolist() == [0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0xFE]
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001], np.uint32).view(np.float32)
    assert fo.e4m3_encode(nan).tolist() == [0x7F, 0xFF, 0x7F, 0xFF]


def test_bf16_rounding_matches_torch():
    rng = np.random.default_rng(0)
    u = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)
    u = np.concatenate([u, np.uint32([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x00000001,
                                      0x00008000, 0x7F7FFFFF, 0x7F800000, 0xFF800000])])
    x = u.view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = fo.f32_to_bf16_bits(x)
    ok = ~np.isnan(x)
    assert np.array_equal(got[ok], want[ok])
    assert np.isnan(fo.bf16_bits_to_f32(got[~ok])).all()


def test_rows_contract_degenerate_rows():
    f = np.float32
    x = np.zeros((7, 8), f)
    x[0] = [1, -2, 3, 0, 0.5, 448, -7, 0.001]
    x[2] = [1e-37, -1e-37, 0, 0, 1e-37, 0, -0.0, 1e-37]
    x[3, 1] = 2.0 ** -116
    x[4] = x[0]; x[4, 3] = np.nan
    x[5] = x[0]; x[5, 2] = np.inf; x[5, 5] = -np.inf
    x[6] = np.nan
    q, sc = fo.quantize_rows(x)
    amax, inv, _ = fo.row_scales(x)
    assert np.isfinite(inv).all() and sc[1] == 1 and amax[4] == 448 and amax[6] == 0 and sc[6] == 1
    assert sc[2] == sc[3] == f(2.0 ** -116) / f(448) and sc[2] >= np.finfo(f).tiny
    assert q[1].tolist() == [0] * 8
    assert (q[2][[2, 3, 5]] == 0).all() and q[2][6] == 0x80 and (q[2] & 0x7F != 0x7F).all()
    assert q[3][1] == 0x7E
    assert q[4][3] == 0xFF and np.array_equal(np.delete(q[4], 3), np.delete(q[0], 3)) and sc[4] == sc[0]
    assert np.isinf(sc[5]) and q[5][2] == 0xFF and q[5][5] == 0xFF
    assert (q[6] == 0xFF).all()
    y = fo.dequantize_rows(q, sc)
    assert np.isnan(y[4][3]) and np.isfinite(np.delete(y[4], 3)).all()
    assert not np.isfinite(y[5]).any() and np.isnan(y[6]).all()
    assert np.isfinite(y[:4]).all() and np.max(np.abs(y[2] - x[2])) <= 2.0 ** -116 / 28


def test_agrees_with_the_torch_cast_restatement_on_ordinary_rows():
    """Where both apply — finite rows with amax >= 2^-116 — this oracle and the torch-cast
    restatement the older fp8 tests use (tests/test_gpu_fp8.py fp8_rows_oracle) give the same
    bits."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(64, 200, generator=g) * torch.logspace(-30, 30, 64)[:, None])
    x[2] = 0
    x[3, :5] = 1e-30
    for dtype in (torch.float32, torch.bfloat16):
        xf = x.to(dtype).float().numpy()
        amax = np.max(np.abs(xf), axis=1).astype(np.float32)
        inv = np.where(amax > 0, np.float32(448.0) / np.where(amax > 0, amax, 1), np.float32(1)).astype(np.float32)
        v = np.clip((xf * inv[:, None]).astype(np.float32), np.float32(-448), np.float32(448))
        qt = torch.from_numpy(v).to(torch.float8_e4m3fn)
        sc = np.where(amax > 0, amax / np.float32(448.0), np.float32(1)).astype(np.float32)
        deq = (qt.float().numpy() * sc[:, None]).astype(np.float32)
        q, s = fo.quantize_rows(xf)
        assert np.array_equal(q, qt.view(torch.uint8).numpy()) and np.array_equal(s, sc)
        assert np.array_equal(fo.dequantize_rows(q, s).view(np.uint32), deq.view(np.uint32))
        want16 = torch.from_numpy(deq).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(fo.dequantize_rows(q, s, "bfloat16"), want16)
