"""The fused NorMuon passes N1, N2 and N3 (csrc/zs_muon.hip), pass by pass, each against float64
formed from what the kernel itself left one pass earlier (O, v and rowstep read back).

Bounds, in units of u = 2^-24, all relative (every operand of the sums is non-negative):
  v after N2: K = 12.  The lane's fp32 chain over the 8 squares of a 16-byte piece (the squares of
    bf16 values are exact, their sum takes at most 8 roundings; the doubles above add 2^-53s), the
    mean's one rounding to fp32, and the lerp's three (the weight, the difference, the fma).
  rowstep: K = 5.  q = fp32(fp32(sqrt v) + fp32(norm_eps)) is within 2 u of the double q; F, the root
    of a sum of rowsq / q^2, inherits 2 u; the quotient's one rounding to fp32.
  the parameter after N3: half an fp32 ulp of rowstep_i O_ij + fp32(p dec), one more ulp where the
    split residual is 0x7FFF (as the Muon test allows for P)."""
import numpy as np
import pytest
import torch

import _muon_oracle as mo
from test_gpu_muon_kernel import _bits, _Table

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (72, 1036): wide, C no multiple of 8 -- the masked tail and N3's element path; (136, 1544): a lane
# walks several loads of a row; (1100, 72): tall, O from XT[cur] with the short stride, lanes idle;
# (300, 64): more rows than N2's 256 threads
SHAPES = [(72, 1036), (136, 1544), (1100, 72), (300, 64)]
STORAGES = ["f32", "bf16copy", "split"]
# shape, fp32 gradient?, storage, v starts at random positive values?, matrix 0 all zero?
CASES = [(s, (i + j) % 2 == 0, st, (i + j) % 2 == 1, False)
         for i, s in enumerate(SHAPES) for j, st in enumerate(STORAGES)]
CASES += [(SHAPES[0], False, "f32", False, False), (SHAPES[2], True, "split", True, False),
          (SHAPES[3], True, "f32", True, True)]


@pytest.mark.parametrize("shape,g32,storage,v_random,zero", CASES)
def test_normuon_passes(gpu, shape, g32, storage, v_random, zero):
    from zero_amd import _lib, kernels

    t = _Table(shape, g32, storage, gpu)
    if zero:  # matrix 0: gradient and buffer all zero, so O = 0 and F = 0
        t.cut(t.d_g, 0).zero_()
        t.cut(t.d_buf, 0).zero_()
    rng = np.random.default_rng(11)
    v0 = [(rng.random(s[0]) * 2e-3 * v_random).astype(np.float32) for s in t.shapes]
    d_v = [torch.from_numpy(v.copy()).to(gpu) for v in v0]
    hpd = dict(lr=0.02, weight_decay=0.1, beta2=0.95, norm_eps=1e-8)
    hp = kernels.normuon_hparams(**hpd)
    mset = kernels.MuonSet(t.rows(), _lib.ZS_F32 if g32 else _lib.ZS_BF16,
                           _lib.ZS_BF16_SPLIT if storage == "split" else _lib.ZS_BF16)
    plain = mset.scratch_bytes
    mset.attach_rows([v.data_ptr() for v in d_v])
    R, C = shape
    assert mset.scratch_bytes == plain + 2 * R * 12 and mset.batch(0)["count"] == 2
    st = torch.cuda.current_stream()
    for which in (0, 1, 2, 3, 4):  # M1, M2, the products (Muon's, pinned there), N1, N2
        mset.run_normuon_pass(hp, which, st, batch=0)
    O = mset.read(0, "XT" if R > C else "X", st).cpu().double().numpy()
    rowsq = mset.read(0, "rowsq", st).cpu().numpy()
    rowstep = mset.read(0, "rowstep", st).cpu().numpy()
    before = t.master().astype(np.float64)
    mset.run_normuon_pass(hp, 5, st, batch=0)  # N3
    torch.cuda.synchronize()
    after = t.master()
    dec = np.float32(1.0 - hpd["lr"] * hpd["weight_decay"])
    for k, i in enumerate((0, 2)):
        v = d_v[i].cpu().numpy().astype(np.float64)
        want_v = mo.lerp(v0[i].astype(np.float64), (O[k] ** 2).mean(axis=1), 1 - hpd["beta2"])
        err_v = np.abs(v - want_v) / np.maximum(want_v, 1e-300)
        q = np.sqrt(v) + hpd["norm_eps"]
        f2 = float((rowsq[k] / q ** 2).sum())
        want_s = np.zeros(R) if f2 == 0 else -(0.2 * hpd["lr"] * np.sqrt(R * C)) / (np.sqrt(f2) * q)
        err_s = np.abs(rowstep[k] - want_s) / np.maximum(np.abs(want_s), 1e-300)
        print(f"{shape} matrix {k}: v {err_v.max() / U:.2f} u (bound 12), rowstep {err_s.max() / U:.2f} u (bound 5)")
        assert np.all(np.abs(v - want_v) <= 12 * U * want_v * (1 + 1e-6))
        assert np.all(np.abs(rowstep[k] - want_s) <= 5 * U * np.abs(want_s) * (1 + 1e-6))
        if zero and k == 0:  # F = 0: every step is +0.0 and the parameter only decays
            assert f2 == 0 and not rowstep[k].any() and not np.signbit(rowstep[k]).any()
        pd = (t.cut(before, i).astype(np.float32) * dec).astype(np.float64)  # the fp32 product
        ref = rowstep[k].astype(np.float64)[:, None] * O[k] + pd
        got = t.cut(after, i)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        slack = 0.5 * ulp
        if storage == "split":  # residual 0x7FFF: the tie the encoding cannot hold, 1 ulp toward zero
            slack = slack + ulp * (t.cut(t.d_lo.cpu().numpy(), i) == 0x7FFF)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= slack * (1 + 1e-9))
        if storage == "bf16copy":
            assert np.array_equal(_bits(t.cut(t.d_copy, i)), _bits(torch.from_numpy(got.copy()).bfloat16()))
    assert np.array_equal(t.cut(after, 1), t.cut(t.p, 1))  # the other batch was not applied
    assert np.array_equal(d_v[1].cpu().numpy(), v0[1])
