"""The fused APOLLO kernels through zero_amd.kernels.ApolloSet: three steps with update_proj_gap=2
(step 3 runs under a new sigma), each stage against float64 formed from what the kernel itself
left one stage earlier.

Bounds, in units of u = 2^-24:
  S: K_s u c sum_k |bf16 g| with K_s = 16 + 4 ceil(K / 64) + (ncut - 1) + 2.  Every product
    sigma * bf16 g is exact; a term passes through at most the 16 roundings inside its own MFMA and
    one per later MFMA of its cut's chain (4 per 64-k stage, padding included; at most those of the
    whole K), the ncut - 1 additions of the cuts' slots, then the rounding of c = fp32(1 / sqrt(rank))
    and of the product with it.
  exp_avg, exp_avg_sq: 0, the fp32 restatement applied to the kernel's own S.
  a_c: K_A = 29 relative, against the double formula on the kernel's own M, V, S and g.  Nh takes 8
    (1 - beta1^t rounded and its division: 2; sqrt V, sqrt(1 - beta2^t) rounded, its division, eps
    rounded and added, all terms positive: 5; the last division: 1), its square 16, the fma chain
    over a 16-byte piece 4: sum Nh^2 20, its root 10.  sum S^2: the chain's 4, root 2.  sum g^2: a
    chain of at most 8: 8.  F^2 = sum s_c^2 gg_c: 2 * 12 + 8 = 32, F 16, so lam at most 16; a_c =
    12 + 16 + its own rounding = 29.
  scaled_grad_norm: K_F = 17 relative (F's 16 and the rounding to fp32).
  the parameter: half an fp32 ulp of a_c g + fp32(p dec) given the kernel's a_c, one more ulp
    where the split residual is 0x7FFF (the tie the encoding cannot hold)."""
import numpy as np
import pytest
import torch

import _apollo_oracle as ao
from oracle import c_oracle

pytestmark = pytest.mark.gpu

U, K_A, K_F = 2.0 ** -24, 29, 17
HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, scale=2.0, update_proj_gap=2,
          norm_growth=1.01)
# tall and wide with K of two hash words plus 8; rows that are no 16-byte multiple (element accesses,
# a padded K); more than one channel tile and K step; one row; a batch; K in two cuts (576 + a ragged
# 456 / 454), tall with 16-byte accesses and wide with element accesses
SHAPES = [[(130, 72)], [(72, 130)], [(257, 33)], [(33, 257)], [(300, 200)], [(1, 40)], [(130, 72)] * 3,
          [(1100, 1032)], [(1030, 1100)]]
IDS = ["130x72", "72x130", "257x33", "33x257", "300x200", "1x40", "3x130x72", "1100x1032", "1030x1100"]
NCUT = {(1100, 1032): 2, (1030, 1100): 2}  # (every other shape: 1)
RANKS = [1, 32, 48, 256]
ENC = [(False, "split"), (False, "f32"), (True, "f32"), (True, "split")]
SEED = 5


def _bf16r(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def exact_grads(rng, shape):
    return rng.integers(-8, 9, shape).astype(np.float32) / 8


def random_grads(rng, shape):  # normal, scaled per row over four decades
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-4, 0, (shape[0], 1))).astype(np.float32)


class _Table:
    """One entry per shape, each stream a tensor of its own."""

    def __init__(self, shapes, rank, g32, storage, gpu):
        from zero_amd import _lib
        from zero_amd.kernels import ApolloSet

        self.shapes, self.rank, self.g32, self.storage, self.gpu = shapes, rank, g32, storage, gpu
        rng = np.random.default_rng(5)
        self.d, rows = [], []
        for i, (R, C) in enumerate(shapes):
            p = (rng.standard_normal((R, C)) * 0.05).astype(np.float32)
            d = {"g": torch.zeros(R, C, dtype=torch.float32 if g32 else torch.bfloat16, device=gpu),
                 "m": torch.zeros(max(R, C), rank, device=gpu), "v": torch.zeros(max(R, C), rank, device=gpu),
                 "f": torch.zeros(1, device=gpu)}
            if storage == "split":
                hi, lo = c_oracle.split_master(p.reshape(-1))
                d["hi"] = torch.from_numpy(hi.view(np.int16).reshape(R, C)).to(gpu)
                d["lo"] = torch.from_numpy(lo.view(np.int16).reshape(R, C)).to(gpu)
                mst, mo, po = d["hi"].data_ptr(), d["lo"].data_ptr(), d["hi"].data_ptr()
            else:
                d["p"], po = torch.from_numpy(p).to(gpu), 0
                mst = mo = d["p"].data_ptr()
            rows.append([d["g"].data_ptr(), mst, mo, po, d["m"].data_ptr(), d["v"].data_ptr(),
                         d["f"].data_ptr(), R, C, SEED + i, i])
            self.d.append(d)
        self.aset = ApolloSet(np.array(rows, np.uint64), _lib.ZS_F32 if g32 else _lib.ZS_BF16,
                              _lib.ZS_BF16_SPLIT if storage == "split" else _lib.ZS_BF16, rank=rank)
        assert self.aset.channels == sum(max(s) for s in shapes)

    def set_grads(self, grads):
        for d, g in zip(self.d, grads):
            d["g"].copy_(torch.from_numpy(g))
        return [g if self.g32 else _bf16r(g) for g in grads]  # what the kernel reads

    def host(self):
        out = []
        for d in self.d:
            h = {k: v.cpu().numpy() for k, v in d.items() if k != "g"}
            if self.storage == "split":
                h["lo"] = h["lo"].view(np.uint16)
                h["p"] = ((h["hi"].view(np.uint16).astype(np.uint32) << 16)
                          + h["lo"].view(np.int16).astype(np.int32).view(np.uint32)).view(np.float32)
            out.append(h)
        return out

    def step(self, t, **hp):
        """One run: (state after, a_c per entry, S per entry as the kernel formed it)."""
        from zero_amd.kernels import apollo_hparams

        st = torch.cuda.current_stream()
        kw = {**HP, **hp}
        self.aset.run(apollo_hparams(**kw), t, st)
        a, sk = self.aset.read("a", st).cpu().numpy(), self.aset.read("sketch", st).cpu().numpy()
        pad = [(NCUT.get(s, 1) * max(s) * self.rank + 3) // 4 * 4 for s in self.shapes]
        assert sum(pad) == self.aset.sketch_elems  # one slot per cut
        c, S = np.float32((-1.0 if kw.get("maximize") else 1.0) / np.sqrt(self.rank)), []
        for o, s in zip(np.cumsum([0] + pad), self.shapes):  # the cuts' slots added in order, in fp32
            slots = sk[o:o + NCUT.get(s, 1) * max(s) * self.rank].reshape(-1, max(s), self.rank)
            total = slots[0]
            for x in slots[1:]:
                total = total + x
            S.append(total * c)
        return self.host(), np.split(a, np.cumsum([max(s) for s in self.shapes])[:-1]), S


def _check_step(tab, before, after, a, S, grads, t, hp):
    """Every stage of one step of every entry; the measured maxima in units of their bounds."""
    worst = dict(S=0.0, a=0.0, F=0.0)
    dec, sgn = np.float32(1.0 - hp["lr"] * hp["weight_decay"]), -1.0 if hp.get("maximize") else 1.0
    for i, ((R, C), g) in enumerate(zip(tab.shapes, grads)):
        G, K = sgn * ao.channels(g).astype(np.float64), min(R, C)
        Gb = sgn * ao.channels(_bf16r(g)).astype(np.float64)
        sig = ao.sigma(K, tab.rank, SEED + i, (t - 1) // hp["update_proj_gap"])
        c = float(np.float32(1.0 / np.sqrt(tab.rank)))
        bound = (16 + 4 * ((K + 63) // 64) + NCUT.get((R, C), 1) - 1 + 2) * U * c * np.abs(Gb).sum(1, keepdims=True)
        err = np.abs(S[i].astype(np.float64) - (Gb @ sig) * c)
        worst["S"] = max(worst["S"], float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (R, C)
        M, V = ao.moments32(before[i]["m"], before[i]["v"], S[i], hp["beta1"], hp["beta2"])
        assert np.array_equal(after[i]["m"].view(np.uint32), M.view(np.uint32)), (R, C)
        assert np.array_equal(after[i]["v"].view(np.uint32), V.view(np.uint32)), (R, C)
        want_a, want_f, _ = ao.scalars(M.astype(np.float64), V.astype(np.float64), S[i].astype(np.float64),
                                       (G ** 2).sum(1), float(before[i]["f"][0]), t, **hp)
        ea = np.abs(a[i] - want_a) / np.maximum(np.abs(want_a), 1e-300)
        ef = abs(float(after[i]["f"][0]) - want_f) / max(want_f, 1e-300)
        worst["a"], worst["F"] = max(worst["a"], float(ea.max()) / U), max(worst["F"], ef / U)
        assert np.all(ea <= K_A * U) and ef <= K_F * U, (R, C)
        upd = a[i].astype(np.float64)[:, None] * G
        ref = (upd if R >= C else upd.T) + (before[i]["p"] * dec).astype(np.float64)
        slack = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        if tab.storage == "split":
            slack = slack * (1 + 2 * (after[i]["lo"] == 0x7FFF))
        assert np.all(np.abs(after[i]["p"].astype(np.float64) - ref) <= slack * (1 + 1e-9)), (R, C)
    return worst


@pytest.mark.parametrize("g32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("rank", RANKS)
@pytest.mark.parametrize("shapes", SHAPES, ids=IDS)
def test_exact_sketch_bit_for_bit(gpu, shapes, rank, g32):
    """Gradients in {-8..8} / 8: every partial sum is exact in fp32 in any order, so with beta1 = 0
    exp_avg is S and must equal fp32(sum) * fp32(1 / sqrt(rank)) bit for bit."""
    tab, rng = _Table(shapes, rank, g32, "f32", gpu), np.random.default_rng(1)
    c, V = np.float32(1.0 / np.sqrt(rank)), [np.zeros((max(s), rank), np.float32) for s in shapes]
    for t in (1, 2, 3):
        grads = tab.set_grads([exact_grads(rng, s) for s in shapes])
        after, _, _ = tab.step(t, beta1=0.0)
        for i, g in enumerate(grads):
            G = ao.channels(g).astype(np.float64)
            S = (G @ ao.sigma(G.shape[1], rank, SEED + i, (t - 1) // 2)).astype(np.float32) * c
            assert np.array_equal(after[i]["m"].view(np.uint32), S.view(np.uint32)), (shapes[i], t)
            _, V[i] = ao.moments32(S, V[i], S, 0.0, HP["beta2"])
            assert np.array_equal(after[i]["v"].view(np.uint32), V[i].view(np.uint32)), (shapes[i], t)


@pytest.mark.parametrize("g32,storage", ENC, ids=["bf16-split", "bf16-f32", "f32-f32", "f32-split"])
@pytest.mark.parametrize("rank,scale_type", [(1, "tensor"), (48, "channel"), (256, "channel"), (32, "tensor")])
@pytest.mark.parametrize("shapes", SHAPES, ids=IDS)
def test_three_steps_match_float64(gpu, shapes, rank, scale_type, g32, storage):
    tab, rng = _Table(shapes, rank, g32, storage, gpu), np.random.default_rng(2)
    hp, before = {**HP, "scale_type": scale_type, "maximize": rank == 48}, None
    for t in (1, 2, 3):
        grads = tab.set_grads([random_grads(rng, s) for s in shapes])
        before = before or tab.host()
        after, a, S = tab.step(t, scale_type=scale_type, maximize=hp["maximize"])
        worst = _check_step(tab, before, after, a, S, grads, t, hp)
        print(f"{shapes[0]} x{len(shapes)} rank {rank} t={t}: S {worst['S']:.3f} of its bound, "
              f"a {worst['a']:.2f} u (bound {K_A}), F {worst['F']:.2f} u (bound {K_F})")
        if scale_type == "tensor":  # one step for every channel of a matrix
            assert all(np.all(x == x[0]) for x in a)
        before = after


@pytest.mark.parametrize("norm_growth", [1.01, 0.0])
def test_the_limiter(gpu, norm_growth):
    """The gradient grows by 4 at step 2: lam > 1 and F_prev holds F / lam; norm_growth=0: lam = 1.
    (beta1 = 0: F is invariant to the gradient's scale but for the moments' memory, and with the
    default beta1 the first moment's lag shrinks Nh at step 2, so F would fall and lam stay 1; without
    it Nh grows by 4 / sqrt((0.000999 + 0.016) / 0.001999) = 1.37.)"""
    shapes = [(130, 72)]
    tab, rng = _Table(shapes, 32, False, "split", gpu), np.random.default_rng(3)
    g1 = random_grads(rng, shapes[0])
    hp = {**HP, "norm_growth": norm_growth, "beta1": 0.0}
    before = tab.host()
    for t, g in ((1, g1), (2, 4 * g1)):
        grads = tab.set_grads([g])
        after, a, S = tab.step(t, norm_growth=norm_growth, beta1=0.0)
        _check_step(tab, before, after, a, S, grads, t, hp)
        G = ao.channels(grads[0]).astype(np.float64)
        _, _, lam = ao.scalars(after[0]["m"].astype(np.float64), after[0]["v"].astype(np.float64),
                               S[0].astype(np.float64), (G ** 2).sum(1), float(before[0]["f"][0]), t, **hp)
        assert (lam > 1.2) == (t == 2 and norm_growth > 0) and (lam == 1.0) == (t == 1 or norm_growth == 0)
        before = after


def test_an_all_zero_gradient_only_decays(gpu):
    tab = _Table([(130, 72), (33, 257)], 48, False, "f32", gpu)
    before = tab.host()
    after, a, _ = tab.step(1)
    dec = np.float32(1.0 - HP["lr"] * HP["weight_decay"])
    for b, h, x in zip(before, after, a):
        assert np.array_equal(h["p"], b["p"] * dec) and np.isfinite(x).all() and np.isfinite(h["f"]).all()
        assert not h["m"].any() and not h["v"].any()


def test_a_nan_stays_inside_its_matrix_and_runs_repeat(gpu):
    shapes, runs = [(130, 72)] * 3, []
    for plant in (False, False, True):
        tab, rng = _Table(shapes, 32, False, "split", gpu), np.random.default_rng(4)
        grads = [random_grads(rng, s) for s in shapes]
        if plant:
            grads[1][77, 5] = np.nan
        tab.set_grads(grads)
        runs.append(tab.step(1)[:2])
    (h0, a0), (h1, a1), (h2, a2) = runs
    same = lambda x, y: all(np.array_equal(x[k], y[k], equal_nan=True) for k in ("m", "v", "f", "p"))  # noqa: E731
    assert all(same(x, y) for x, y in zip(h0, h1)) and all(np.array_equal(x, y) for x, y in zip(a0, a1))
    assert np.isnan(a2[1][77]) and np.isnan(h2[1]["p"][77]).all() and np.isnan(h2[1]["f"]).all()
    assert all(same(h0[i], h2[i]) and np.array_equal(a0[i], a2[i]) for i in (0, 2))
