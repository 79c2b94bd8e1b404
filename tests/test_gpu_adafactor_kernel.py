"""The fused Adafactor kernels through zero_amd.kernels.AdafactorSet: one step from a planted state
against tests/_adafactor_oracle.py on the widened inputs.  DESIGN.md §4 "Fused Adafactor" counts the
fp32 roundings: K_S = 21 + 1 (factors, relative), K = 82 + 1 (0.5 ulp32(ref) + K * 2^-24 * |delta|).
A split master stored as residual 0x7FFF (the tie the encoding cannot hold) sits 1 ulp toward zero
by design and is allowed that ulp."""
import numpy as np
import pytest
import torch

import _adafactor_oracle as ao
from oracle import c_oracle

pytestmark = pytest.mark.gpu

K_S, K = 22, 83
SHAPES = [(37, 53), (70, 520), (1, 300), (300, 1), (4100, 8), (3, 4104), (2, 33, 40), (1000,), (63,),
          (40, 48), (16, 24)]  # the last two: a zero row and column of g; an all-zero parameter
STORAGE = ("f32", "bf16copy", "split")
HP = dict(lr=1e-2, beta2_decay=-0.8, eps2=1e-3, d=1.0)
SLACK = 192


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _join(hi, lo):
    return ((hi.astype(np.uint32) << 16) + lo.view(np.int16).astype(np.int32).view(np.uint32)).view(np.float32)


class _Case:
    """All of ``shapes`` in one table, each at a 64-element boundary of flat arrays, SLACK apart."""
    def __init__(self, shapes, g32, storage, scale, t, seed=7):
        self.shapes, self.g32, self.storage, self.t = shapes, g32, storage, t
        rng = np.random.default_rng(seed)
        self.off, self.soff, n, s = [], [], 0, 0
        for sh in shapes:
            self.off.append(n)
            n += (int(np.prod(sh)) + SLACK + 63) // 64 * 64
            self.soff.append(s)
            s += (int(np.prod(sh[:-1])) + int(np.prod(sh[:-2] + sh[-1:])) if len(sh) > 1 else sh[0]) + 8
        self.N, self.S = n, s
        p = (rng.standard_normal(n) * 0.05).astype(np.float32)
        g = (rng.standard_normal(n) * scale).astype(np.float32)
        for sh, o in zip(shapes, self.off):
            if sh == (40, 48):
                gv = g[o:o + 1920].reshape(sh)
                gv[3, :], gv[:, 5] = 0.0, 0.0
            if sh == (16, 24):
                p[o:o + 384] = 0.0
        self.state = (rng.random(s) * 1e-4 * scale * scale).astype(np.float32) if t > 1 else np.zeros(s, np.float32)
        self.g = g if g32 else _bf16(g)
        if storage == "split":
            self.hi, self.lo = c_oracle.split_master(p)
            p = _join(self.hi, self.lo)
        self.p = p

    def _views(self, i, state):
        sh, so = self.shapes[i], self.soff[i]
        if len(sh) == 1:
            return {"variance": state[so:so + sh[0]]}
        nr, nc = int(np.prod(sh[:-1])), int(np.prod(sh[:-2] + sh[-1:]))
        return {"row_var": state[so:so + nr].reshape(sh[:-1] + (1,)),
                "col_var": state[so + nr:so + nr + nc].reshape(sh[:-2] + (1, sh[-1]))}

    def reference(self):
        gw = self.g.astype(np.float64) if self.g32 else \
            (self.g.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        out = []
        for i, (sh, o) in enumerate(zip(self.shapes, self.off)):
            n = int(np.prod(sh))
            out.append(ao.step(self.p[o:o + n].reshape(sh), gw[o:o + n].reshape(sh),
                               self._views(i, self.state), self.t, **HP))
        return out

    def run(self, gpu):
        from zero_amd import _lib
        from zero_amd.kernels import AdafactorSet, adafactor_hparams

        dev = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.copy()).to(gpu)  # noqa: E731
        T = {"g": dev(self.g), "state": dev(self.state)}
        if self.storage == "split":
            T["hi"], T["lo"] = dev(self.hi), dev(self.lo)
        else:
            T["p"] = dev(self.p)
            if self.storage == "bf16copy":
                T["pb"] = torch.zeros(self.N, dtype=torch.int16, device=gpu)
        gsz = 4 if self.g32 else 2
        rows = []
        for i, (sh, o) in enumerate(zip(self.shapes, self.off)):
            R, C = (1, sh[0]) if len(sh) == 1 else sh[-2:]
            B = int(np.prod(sh[:-2])) if len(sh) > 2 else 1
            for b in range(B):
                e, so = o + b * R * C, self.soff[i]
                if self.storage == "split":
                    mst, mo, po = T["hi"].data_ptr() + 2 * e, T["lo"].data_ptr() + 2 * e, T["hi"].data_ptr() + 2 * e
                else:
                    mst = mo = T["p"].data_ptr() + 4 * e
                    po = T["pb"].data_ptr() + 2 * e if self.storage == "bf16copy" else 0
                rv = T["state"].data_ptr() + 4 * (so + b * R)
                cv = 0 if len(sh) == 1 else T["state"].data_ptr() + 4 * (so + B * R + b * C)
                rows.append([T["g"].data_ptr() + gsz * e, mst, mo, po, rv, cv, R, C, i])
        aset = AdafactorSet(np.array(rows, np.uint64), _lib.ZS_F32 if self.g32 else _lib.ZS_BF16,
                            _lib.ZS_BF16_SPLIT if self.storage == "split" else _lib.ZS_BF16)
        aset.run(adafactor_hparams(HP["lr"], HP["beta2_decay"], (None, HP["eps2"]), HP["d"]), self.t,
                 torch.cuda.current_stream(gpu))
        torch.cuda.synchronize(gpu)
        return {k: v.cpu().numpy() for k, v in T.items()}


def _check(case, got, ref):
    touched = np.zeros(case.N, bool)
    s_touched = np.zeros(case.S, bool)
    master = _join(got["hi"].view(np.uint16), got["lo"].view(np.uint16)) if case.storage == "split" else got["p"]
    for i, (sh, o) in enumerate(zip(case.shapes, case.off)):
        n = int(np.prod(sh))
        want_p, want_state, delta = ref[i]
        touched[o:o + n] = True
        tol = 0.5 * np.spacing(np.abs(want_p).astype(np.float32)).astype(np.float64) + K * 2.0 ** -24 * np.abs(delta)
        if case.storage == "split":  # the tie the encoding stores 1 ulp toward zero
            clamped = (got["lo"][o:o + n].view(np.uint16) == 0x7FFF).reshape(sh)
            tol = tol + clamped * np.spacing(np.abs(want_p).astype(np.float32))
        err = np.abs(master[o:o + n].reshape(sh).astype(np.float64) - want_p)
        assert (err <= tol).all(), (sh, float(np.max(err / tol)))
        for name, view in case._views(i, got["state"]).items():
            want = want_state[name]
            serr = np.abs(view.astype(np.float64) - want)
            print(f"{sh}: {name} max rel err {np.max(serr / np.maximum(want, 1e-300)) * 2.0 ** 24:.2f} * 2^-24")
            assert (serr <= K_S * 2.0 ** -24 * want).all(), (sh, name)
            s_touched[case.soff[i]:case.soff[i] + sum(v.size for v in case._views(i, got["state"]).values())] = True
    # the bf16 copy is the RNE of the stored master, bit for bit
    copy = got.get("pb", got.get("hi"))
    if copy is not None:
        assert np.array_equal(copy.view(np.uint16)[touched], _bf16(master)[touched])
    # every byte outside what the step may write is untouched
    assert np.array_equal(got["g"].view(np.uint8), case.g.view(np.uint8))
    assert np.array_equal(got["state"][~s_touched], case.state[~s_touched])
    if case.storage == "split":
        assert np.array_equal(got["hi"].view(np.uint16)[~touched], case.hi[~touched])
        assert np.array_equal(got["lo"].view(np.uint16)[~touched], case.lo.view(np.uint16)[~touched])
    else:
        assert np.array_equal(got["p"][~touched].view(np.uint32), case.p[~touched].view(np.uint32))
        if "pb" in got:
            assert not got["pb"][~touched].any()


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("scale", [1.0, 1e-3])
@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("g32", [False, True], ids=["g_bf16", "g_f32"])
def test_one_step_matches_the_oracle(gpu, g32, storage, scale, t):
    case = _Case(SHAPES, g32, storage, scale, t)
    got = case.run(gpu)
    _check(case, got, case.reference())
    again = case.run(gpu)  # the same bits from run to run
    assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)
