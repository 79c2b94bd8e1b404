"""The fused Adam-mini kernels through zero_amd.kernels.AdamMiniSet: two steps (t = 1, 2) from a
planted state, each against float64 formed from what the kernel itself left one stage earlier.

Bounds, in units of u = 2^-24, relative (every operand of the sums is non-negative):
  block_exp_avg_sq: K_v = 15, the plain count of the fp32 roundings on the path.  g / 3 rounds once,
    which its square doubles (2; the square itself is not rounded, it sits inside an fma); the fma
    chain over the 8 elements of a 16-byte bf16 piece rounds 8 times (4 for fp32 gradients; the
    doubles above add 2^-53s); the mean's one rounding to fp32 (1); v * beta2 and the fma (2); the
    host scalars beta2 and 1 - beta2 (2).
  a_b: 1, the one rounding of the double formula applied to the kernel's own v_b.
  the parameter: half an fp32 ulp of a_b m + fp32(p dec) given the kernel's a_b and m, one more
    ulp where the split residual is 0x7FFF (the tie the encoding cannot hold)."""
import numpy as np
import pytest
import torch

import _adamini_oracle as ao
from oracle import c_oracle

pytestmark = pytest.mark.gpu

U, K_V, CAP, DIV = 2.0 ** -24, 15, 16384, 3.0
HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)
# one piece per thread; one piece past a round of 256; a row shorter than a wave; odd C (the element
# path); block_rows=2; the last resident and the first two-pass block; one block of several tiles;
# 1-D, resident and two-pass
SHAPES = [((5, 2048), 1), ((3, 2056), 1), ((7, 72), 1), ((4, 1037), 1), ((6, 1544), 2),
          ((2, CAP), 1), ((2, CAP + 8), 1), ((300, 64), 0), ((1000,), 1), ((40000,), 1)]
ENC = [(False, "split"), (False, "bf16copy"), (True, "f32")]
OTHER = ((3, 40), 1)  # the entry between the two of the shape under test
SLACK = 192


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _join(hi, lo):
    return ((hi.astype(np.uint32) << 16) + lo.view(np.int16).astype(np.int32).view(np.uint32)).view(np.float32)


class _Table:
    """Three entries in flat arrays, each at a 64-element boundary, SLACK elements of poison apart."""

    def __init__(self, shape, br, g32, storage, gpu, cap, edit_g=None):
        from zero_amd import _lib
        from zero_amd.kernels import AdamMiniSet

        self.ents, self.g32, self.storage = [(shape, br), OTHER, (shape, br)], g32, storage
        rng = np.random.default_rng(5)
        self.off, self.voff, n, nv = [], [], SLACK, 4
        for sh, b in self.ents:
            self.off.append(n), self.voff.append(nv)
            n += (int(np.prod(sh)) + SLACK + 63) // 64 * 64
            nv += ao.blocks(sh, b) + 4
        g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        if edit_g is not None:
            edit_g(g, self.off)
        p = (rng.standard_normal(n) * 0.05).astype(np.float32)
        host = {"g": g if g32 else _bf16(g), "m": (rng.standard_normal(n) * 1e-3).astype(np.float32),
                "v": (rng.random(nv) * 1e-4).astype(np.float32)}
        if storage == "split":
            host["hi"], host["lo"] = c_oracle.split_master(p)
        else:
            host["p"] = p
            if storage == "bf16copy":
                host["pb"] = np.full(n, 0x7FC1, np.uint16)
        self.d = {k: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.copy()).to(gpu)
                  for k, a in host.items()}
        d, gsz, rows = self.d, 4 if g32 else 2, []
        for i, ((sh, b), o, vo) in enumerate(zip(self.ents, self.off, self.voff)):
            if storage == "split":
                mst, mo = d["hi"].data_ptr() + 2 * o, d["lo"].data_ptr() + 2 * o
                po = mst
            else:
                mst = mo = d["p"].data_ptr() + 4 * o
                po = d["pb"].data_ptr() + 2 * o if storage == "bf16copy" else 0
            R = 1 if len(sh) < 2 else sh[0]
            rows.append([d["g"].data_ptr() + gsz * o, mst, mo, po, d["m"].data_ptr() + 4 * o,
                         d["v"].data_ptr() + 4 * vo, R, int(np.prod(sh)) // R, b if len(sh) > 1 else 0, i])
        self.aset = AdamMiniSet(np.array(rows, np.uint64), _lib.ZS_F32 if g32 else _lib.ZS_BF16,
                                _lib.ZS_BF16_SPLIT if storage == "split" else _lib.ZS_BF16, resident_cap=cap)
        assert self.aset.blocks == sum(ao.blocks(sh, b) for sh, b in self.ents)

    def host(self):
        h = {k: v.cpu().numpy() for k, v in self.d.items()}
        h = {k: (v.view(np.uint16) if v.dtype == np.int16 else v) for k, v in h.items()}
        h["master"] = _join(h["hi"], h["lo"]) if self.storage == "split" else h["p"]
        return h

    def step(self, t, **hp):
        from zero_amd.kernels import adamini_hparams

        st = torch.cuda.current_stream()
        self.aset.run(adamini_hparams(**{**HP, **hp}, grad_div=DIV), t, st)
        a = self.aset.read("a", st)
        torch.cuda.synchronize()
        return self.host(), a.cpu().numpy()

    def check(self, before, after, a, t):
        gw = before["g"] if self.g32 else (before["g"].astype(np.uint32) << 16).view(np.float32)
        gavg = (torch.from_numpy(gw) / DIV).numpy()  # fp32, correctly rounded
        dec = np.float32(1.0 - HP["lr"] * HP["weight_decay"])
        touched, vtouched, ab = np.zeros(gw.size, bool), np.zeros(before["v"].size, bool), 0
        for (sh, b), o, vo in zip(self.ents, self.off, self.voff):
            n, nb = int(np.prod(sh)), ao.blocks(sh, b)
            cut = lambda x: x[o:o + n]  # noqa: E731
            touched[o:o + n], vtouched[vo:vo + nb] = True, True
            want_m = torch.from_numpy(cut(before["m"]).copy()).lerp_(torch.from_numpy(cut(gavg).copy()), 1 - HP["beta1"])
            assert np.array_equal(cut(after["m"]).view(np.uint32), want_m.numpy().view(np.uint32)), sh
            _, _, want_v, _ = ao.step(cut(before["master"]).astype(np.float64), cut(gw).astype(np.float64) / DIV,
                                      cut(before["m"]).astype(np.float64), before["v"][vo:vo + nb].astype(np.float64),
                                      t, nb, **HP)
            v = after["v"][vo:vo + nb].astype(np.float64)
            want_a = -(HP["lr"] / (1 - HP["beta1"] ** t)) / (np.sqrt(v) / np.sqrt(1 - HP["beta2"] ** t) + HP["eps"])
            got_a = a[ab:ab + nb].astype(np.float64)
            ab += nb
            print(f"{sh} t={t}: v {np.max(np.abs(v - want_v) / want_v) / U:.2f} u (bound {K_V}), "
                  f"a {np.max(np.abs(got_a - want_a) / np.abs(want_a)) / U:.2f} u (bound 1)")
            assert np.all(np.abs(v - want_v) <= K_V * U * want_v * (1 + 1e-6)), sh
            assert np.all(np.abs(got_a - want_a) <= U * np.abs(want_a) * (1 + 1e-6)), sh
            pd = (cut(before["master"]) * dec).astype(np.float64)  # the fp32 product
            ref = (got_a[:, None] * cut(after["m"]).astype(np.float64).reshape(nb, -1)).reshape(-1) + pd
            ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
            slack = 0.5 * ulp
            if self.storage == "split":
                slack = slack + ulp * (cut(after["lo"]) == 0x7FFF)
            assert np.all(np.abs(cut(after["master"]).astype(np.float64) - ref) <= slack * (1 + 1e-9)), sh
        copy = after.get("pb", after.get("hi"))
        if copy is not None:  # the bf16 copy is the RNE of the stored master, bit for bit
            assert np.array_equal(copy[touched], _bf16(after["master"])[touched])
        for k in before:  # the gradient, and every byte outside the entries, is untouched
            keep = np.ones(before[k].size, bool) if k == "g" else ~(vtouched if k == "v" else touched)
            assert np.array_equal(before[k][keep].view(np.uint8), after[k][keep].view(np.uint8)), k


@pytest.mark.parametrize("cap", [0, CAP])
@pytest.mark.parametrize("g32,storage", ENC, ids=[e[1] for e in ENC])
@pytest.mark.parametrize("shape,br", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_two_steps_match_float64(gpu, shape, br, g32, storage, cap):
    tab = _Table(shape, br, g32, storage, gpu, cap)
    assert (tab.aset.resident_elems > 0) == (cap > 0)
    assert (tab.aset.twopass_elems > 0) == (cap == 0 or int(np.prod(shape)) // ao.blocks(shape, br) > cap)
    before = tab.host()
    for t in (1, 2):
        after, a = tab.step(t)
        tab.check(before, after, a, t)
        before = after


@pytest.mark.parametrize("cap", [0, CAP])
def test_a_nan_stays_inside_its_block(gpu, cap):
    def plant(g, off):
        g[off[0] + 2 * 2048 + 77] = np.nan

    runs = []
    for edit in (None, plant):
        tab = _Table((5, 2048), 1, False, "split", gpu, cap, edit_g=edit)
        after, a = tab.step(1)
        runs.append((tab, after, a))
    (tab, clean, a0), (_, dirty, a1) = runs
    o, bad = tab.off[0], slice(tab.off[0] + 2 * 2048, tab.off[0] + 3 * 2048)
    assert np.isnan(a1[2]) and np.isnan(dirty["master"][bad]).all() and np.isnan(dirty["v"][tab.voff[0] + 2])
    for x in (a0, a1):
        x[2] = 0
    for h in (clean, dirty):
        for k in ("g", "m", "hi", "lo"):
            h[k][bad] = 0
        h["v"][tab.voff[0] + 2] = 0
    assert np.array_equal(a0, a1) and all(np.array_equal(clean[k], dirty[k]) for k in ("m", "v", "hi", "lo"))


@pytest.mark.parametrize("cap", [0, CAP])
def test_an_all_zero_gradient_only_decays(gpu, cap):
    tab = _Table((5, 2048), 1, False, "bf16copy", gpu, cap, edit_g=lambda g, off: g.fill(0.0))
    tab.d["m"].zero_(), tab.d["v"].zero_()
    before = tab.host()
    after, a = tab.step(1)
    assert not after["v"].any() and not after["m"].any()
    assert np.all(a == np.float32(-(HP["lr"] / (1 - HP["beta1"])) / HP["eps"]))
    dec, t = np.float32(1.0 - HP["lr"] * HP["weight_decay"]), np.zeros(before["p"].size, bool)
    for (sh, _), o in zip(tab.ents, tab.off):
        t[o:o + int(np.prod(sh))] = True
    assert np.array_equal(after["p"][t], before["p"][t] * dec) and np.array_equal(after["p"][~t], before["p"][~t])
