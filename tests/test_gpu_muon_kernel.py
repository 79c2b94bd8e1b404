"""The fused Muon kernels (csrc/zs_muon.hip): the bare NT product against the float64 product of the
same bf16 inputs, and one step pass by pass against torch's CPU lerp_, tests/_muon_oracle.py and
torch's own bf16 Newton-Schulz.  The product's bound per element is one bf16 output rounding plus an
fp32 accumulation of K terms: half a bf16 ulp of the reference (it lies in (2^-9 |v|, 2^-8 |v|]: 2^-9
|ref| alone is below what a correctly rounded result can miss by) plus (K + 2) 2^-24 (|alpha| sum
|a||b| + |beta e|)."""
import numpy as np
import pytest
import torch
from torch.optim._muon import _zeropower_via_newtonschulz

import _muon_oracle as mo
from oracle import c_oracle

pytestmark = pytest.mark.gpu

OTHER = (24, 40)
# shape, fp32 gradient?, storage, nesterov, momentum
CASES = [((1, 70), True, "f32", True, 0.95), ((33, 70), False, "split", False, 0.3),
         ((96, 40), True, "bf16copy", True, 0.3), ((128, 128), False, "f32", False, 0.95),
         ((130, 257), True, "split", True, 0.95), ((256, 384), False, "bf16copy", True, 0.95)]
# M, N, K, symmetric?, beta
GEMMS = [(1, 70, 1, False, 0.5), (33, 33, 70, True, -4.775), (40, 96, 40, False, 3.4445),
         (128, 128, 128, True, 0.0), (130, 130, 257, True, -4.775), (130, 257, 130, False, 3.4445),
         (256, 384, 256, False, 0.0), (256, 256, 384, True, 0.5)]


def _half_ulp_bf16(x):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 8)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


@pytest.mark.parametrize("M,N,K,sym,beta", GEMMS)
def test_gemm_nt_against_float64(gpu, M, N, K, sym, beta):
    from zero_amd import kernels

    gen = torch.Generator().manual_seed(M * 1000 + N + K)
    a = (torch.randn(M, K, generator=gen) / K ** 0.5).bfloat16()
    b = a if sym else (torch.randn(N, K, generator=gen) / K ** 0.5).bfloat16()
    e = torch.randn(M, N, generator=gen)
    e = ((e + e.T) / 2 if sym else e).bfloat16()
    alpha = 2.0315
    prod = a.double() @ b.double().T
    ref = alpha * prod + beta * e.double()
    mag = abs(alpha) * (a.double().abs() @ b.double().abs().T) + abs(beta) * e.double().abs()
    bound = _half_ulp_bf16(ref.numpy()) + (K + 2) * 2.0 ** -24 * mag.numpy()
    A, B, E = a.to(gpu), (None if sym else b.to(gpu)), e.to(gpu)
    D = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    D2 = None if sym else torch.full((N, M), float("nan"), dtype=torch.bfloat16, device=gpu)
    kernels.muon_gemm_nt(A, A if sym else B, D, E=E if beta else None, D2=D2, alpha=alpha, beta=beta,
                         sym=sym, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    err = np.abs(D.cpu().double().numpy() - ref.numpy())
    print(f"max err / bound {np.max(err / bound):.3f}; beyond 2^-9 |ref| alone: "
          f"{int((err > 2.0 ** -9 * np.abs(ref.numpy())).sum())} of {err.size}")
    assert np.all(err <= bound)
    mirror = D if sym else D2  # the mirror tile / the transposed store: the same bits
    assert np.array_equal(_bits(mirror), _bits(D).T)


class _Table:
    """Two matrices of ``shape`` around one of OTHER in flat arrays, 64 elements apart."""
    def __init__(self, shape, g32, storage, dev, seed=5):
        rng = np.random.default_rng(seed)
        self.shapes = [shape, OTHER, shape]
        self.off, n = [], 0
        for s in self.shapes:
            self.off.append(n)
            n += (s[0] * s[1] + 127) // 64 * 64
        g = torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 1e-2)
        self.g = g if g32 else g.bfloat16()
        self.buf = torch.from_numpy(rng.standard_normal(n).astype(np.float32) * 1e-2)
        p = (rng.standard_normal(n) * 0.05).astype(np.float32)
        self.storage = storage
        if storage == "split":
            hi, lo = c_oracle.split_master(p)
            self.d_hi = torch.from_numpy(hi.view(np.int16).copy()).to(dev)
            self.d_lo = torch.from_numpy(lo.view(np.int16).copy()).to(dev)
            p = self._join(hi.view(np.int16), lo.view(np.int16))
        self.p = p
        self.d_p = torch.from_numpy(p.copy()).to(dev)
        self.d_copy = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        self.d_g, self.d_buf = self.g.to(dev), self.buf.to(dev)

    @staticmethod
    def _join(hi, lo):
        return ((hi.view(np.uint16).astype(np.uint32) << 16) +
                lo.astype(np.int32).view(np.uint32)).view(np.float32)

    def rows(self):
        out = []
        for i, (s, o) in enumerate(zip(self.shapes, self.off)):
            g = self.d_g.data_ptr() + o * self.d_g.element_size()
            if self.storage == "split":
                m, mo_, po = self.d_hi.data_ptr() + 2 * o, self.d_lo.data_ptr() + 2 * o, \
                    self.d_hi.data_ptr() + 2 * o
            else:
                m = mo_ = self.d_p.data_ptr() + 4 * o
                po = self.d_copy.data_ptr() + 2 * o if self.storage == "bf16copy" else 0
            out.append([g, m, mo_, po, self.d_buf.data_ptr() + 4 * o, s[0], s[1], i])
        return np.array(out, np.uint64)

    def cut(self, flat, i):
        s, o = self.shapes[i], self.off[i]
        return flat[o:o + s[0] * s[1]].reshape(s)

    def master(self):
        if self.storage == "split":
            return self._join(self.d_hi.cpu().numpy(), self.d_lo.cpu().numpy())
        return self.d_p.cpu().numpy()


@pytest.mark.parametrize("shape,g32,storage,nesterov,momentum", CASES)
def test_one_step_pass_by_pass(gpu, shape, g32, storage, nesterov, momentum):
    from zero_amd import _lib, kernels

    t = _Table(shape, g32, storage, gpu)
    hpd = dict(lr=0.02, weight_decay=0.1, momentum=momentum, nesterov=nesterov,
               adjust_lr_fn="match_rms_adamw" if nesterov else None)
    hp = kernels.muon_hparams(**hpd)
    mset = kernels.MuonSet(t.rows(), _lib.ZS_F32 if g32 else _lib.ZS_BF16,
                           _lib.ZS_BF16_SPLIT if storage == "split" else _lib.ZS_BF16)
    st = torch.cuda.current_stream()
    assert mset.batches == 2 and mset.batch(0)["count"] == 2 and mset.batch(1)["count"] == 1
    # M1: the momentum buffer is torch's lerp_ on the widened gradient, bit for bit (all matrices)
    mset.run_pass(hp, 0, st, batch=1)  # (the scratch, the norms in it, holds the batch run last)
    mset.run_pass(hp, 0, st, batch=0)
    gw = t.g.float()
    buf = t.buf.clone().lerp_(gw, 1 - momentum)
    assert all(torch.equal(t.cut(t.d_buf.cpu(), i), t.cut(buf, i)) for i in range(3))
    us = [t.cut(gw.lerp(buf, momentum) if nesterov else buf, i) for i in (0, 2)]
    # M2: X is the oracle's normalised bf16 X, bit for bit, and XT its transpose
    mset.run_pass(hp, 1, st, batch=0)
    X, XT = mset.read(0, "X", st), mset.read(0, "XT", st)
    for k, u in enumerate(us):
        want = torch.from_numpy(mo.normalised(u.double().numpy())).bfloat16()
        assert np.array_equal(_bits(X[k]), _bits(want))
        assert np.array_equal(_bits(XT[k]), _bits(X[k]).T)
    # the iteration: no further from the unrounded one than 1.5 x torch's own bf16 run
    mset.run_pass(hp, 2, st, batch=0)
    tall = shape[0] > shape[1]
    O = mset.read(0, "XT" if tall else "X", st).cpu()
    for k, u in enumerate(us):
        exact = mo.newton_schulz(u.double().numpy())
        theirs = _zeropower_via_newtonschulz(u, mo.COEFFS, 5, 1e-7).double().numpy()
        d_ours = np.linalg.norm(O[k].double().numpy() - exact) / np.linalg.norm(exact)
        d_torch = np.linalg.norm(theirs - exact) / np.linalg.norm(exact)
        print(f"{shape} matrix {k}: ours {d_ours:.4f}, torch {d_torch:.4f}, ratio {d_ours / d_torch:.3f}")
        assert d_ours <= 1.5 * d_torch
    # P: fma(-adjusted lr, O, p * (1 - lr wd)) within half an fp32 ulp, given the kernel's own O
    before = t.master().astype(np.float64)
    mset.run_pass(hp, 3, st, batch=0)
    torch.cuda.synchronize()
    after = t.master()
    alr = np.float32(-mo.adjusted_lr(hpd["lr"], hpd["adjust_lr_fn"], shape))
    dec = np.float32(1.0 - hpd["lr"] * hpd["weight_decay"])
    for k, i in enumerate((0, 2)):
        pd = (t.cut(before, i).astype(np.float32) * dec).astype(np.float64)  # the fp32 product
        ref = np.float64(alr) * O[k].double().numpy() + pd
        got = t.cut(after, i)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        slack = 0.5 * ulp
        if storage == "split":  # residual 0x7FFF: the tie the encoding cannot hold, 1 ulp toward zero
            slack = slack + ulp * (t.cut(t.d_lo.cpu().numpy(), i) == 0x7FFF)
        assert np.all(np.abs(got.astype(np.float64) - ref) <= slack * (1 + 1e-9))
        if storage == "bf16copy":
            assert np.array_equal(_bits(t.cut(t.d_copy, i)), _bits(torch.from_numpy(got.copy()).bfloat16()))
    assert np.array_equal(t.cut(after, 1), t.cut(t.p, 1))  # batch 1 was not applied
