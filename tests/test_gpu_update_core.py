"""``UpdateCore`` (zero_amd/_update.py) on its own, without an engine or a wrapper around it: three
"parameters" of 4099, 64 and 1 elements in two param groups, bf16 with the split master and fp32,
Adam and SGD with momentum.  4099 leaves a 3-element tail behind its vector part and the 1-element
parameter is all tail (the predicated path).  Two geometries: ``packed`` — back to back, L = 4099 +
64 + 1 = 4164, so the second and third start off the vector alignment — and ``aligned`` — every
parameter on a 64-element boundary as the planner and the chunk arena place them, L = 4225, odd, so
the int16 residuals end in half a word ((L + 1) // 2).

Every call is mirrored by the oracles the kernel tests use (oracle/c_oracle.py for Adam,
tests/_sgd_oracle.py for SGD) and compared bit for bit.
"""
import numpy as np
import pytest
import torch

import _sgd_oracle as so
from oracle import c_oracle

pytestmark = pytest.mark.gpu

SIZES = (4099, 64, 1)
GROUP_OF = (0, 1, 0)
OFFSETS = {"packed": (0, 4099, 4163), "aligned": (0, 4160, 4224)}
WS = 2  # the gradient divisor the hyper-parameters carry
COUNTS = (1, 1, 2)  # per-parameter step counts of the calls below


def _groups(kind):
    a, b = torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))
    if kind == "sgd":
        return torch.optim.SGD([{"params": [a], "lr": 0.1, "momentum": 0.9, "weight_decay": 0.01},
                                {"params": [b], "lr": 0.05, "momentum": 0.8, "nesterov": True}], lr=0.1)
    return torch.optim.Adam([{"params": [a], "lr": 1e-2, "weight_decay": 0.1},
                             {"params": [b], "lr": 3e-3, "betas": (0.8, 0.95)}])


def _bits(t):
    """Host bits of a device tensor (bf16 / int16 as uint16)."""
    if t.dtype in (torch.bfloat16, torch.int16):
        return t.view(torch.int16).cpu().numpy().view(np.uint16).copy()
    return t.cpu().numpy().copy()


def _dev(a, dtype, gpu):
    if dtype == torch.bfloat16:
        return torch.from_numpy(a.view(np.int16)).to(gpu).view(torch.bfloat16)
    return torch.from_numpy(a).to(gpu)


class _Ref:
    """The oracle's copy of the shard: per parameter p (fp32, or hi + lo), m, v, vmax."""

    def __init__(self, kind, split, p0):
        self.kind, self.split = kind, split
        self.p = [a.copy() for a in p0]  # fp32 values, or bf16 bits with lo = 0
        self.lo = [np.zeros(a.size, np.uint16) for a in p0]
        self.m = [np.zeros(a.size, np.float32) for a in p0]
        self.v = [np.zeros(a.size, np.float32) for a in p0]
        self.vmax = None

    def step(self, grads, counts, hparams_of):
        for i, g in enumerate(grads):
            h = hparams_of(GROUP_OF[i])
            if self.kind == "sgd":
                hp = so.SgdHP(h["lr"], h["momentum"], h["dampening"], h["weight_decay"],
                              nesterov=h["nesterov"], maximize=h["maximize"],
                              first=counts[i] == 1, grad_div=float(WS))
                if self.split:
                    self.p[i], self.lo[i], self.m[i], _ = so.step_split(self.p[i], self.lo[i], g,
                                                                        self.m[i], hp)
                else:
                    self.p[i], self.m[i], _ = so.step_f32(self.p[i], g, self.m[i], hp)
                continue
            hp = c_oracle.hparams(h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"],
                                  counts[i], decoupled=h["decoupled"], amsgrad=h["amsgrad"],
                                  maximize=h["maximize"], grad_div=float(WS))
            vmax = None if self.vmax is None else self.vmax[i]
            if self.split:
                c_oracle.adam_bf16_split(self.p[i], self.lo[i], g, self.m[i], self.v[i], hp, vmax=vmax)
            else:
                c_oracle.adam_f32(self.p[i], g, self.m[i], self.v[i], hp, vmax=vmax)


@pytest.mark.parametrize("geom", ["packed", "aligned"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("dt", ["bf16_split", "f32"])
def test_core_alone(gpu, dt, kind, geom):
    from zero_amd import _lib
    from zero_amd._sharded import group_hparams
    from zero_amd._update import UpdateCore, state_layout
    from zero_amd.kernels import AdamSet, SgdSet

    split = dt == "bf16_split"
    tdt = torch.bfloat16 if split else torch.float32
    es = 2 if split else 4
    offs = OFFSETS[geom]
    L = offs[-1] + SIZES[-1]
    assert L == {"packed": 4099 + 64 + 1, "aligned": 4225}[geom]
    rng = np.random.default_rng(20 + len(geom) + 2 * split + (kind == "sgd"))

    def draw(scale):  # one array per parameter, in the shard's dtype (bf16: its bits)
        out = [(rng.standard_normal(n) * scale).astype(np.float32) for n in SIZES]
        return [so.f32_to_bf16_bits(a) for a in out] if split else out

    def shard(arrs):  # the parameters' arrays at their offsets of an L-element device buffer
        full = np.zeros(L, np.uint16 if split else np.float32)
        for o, a in zip(offs, arrs):
            full[o:o + a.size] = a
        return _dev(full, tdt, gpu)

    p0, grads, grads2 = draw(1.0), draw(0.1), draw(0.1)
    P, G, G2 = shard(p0), shard(grads), shard(grads2)
    opt = _groups(kind)
    hparams_of = lambda gi: group_hparams(kind, opt.param_groups[gi], opt)  # noqa: E731
    core = UpdateCore(kind, L, gpu, WS, GROUP_OF, len(SIZES), split=split, momentum=True)
    ref = _Ref(kind, split, p0)
    stream = torch.cuda.current_stream(gpu)

    # (a) the views sit where the layout says
    total, lay = state_layout(kind, L, split=split, fp32_master=False, carry=False, momentum=True)
    base = core.state.data_ptr()
    assert core.state.numel() == total and core.state.dtype == torch.float32
    for i, (o, n) in enumerate(zip(offs, SIZES)):
        vw = core.views(o, n, (n,))
        names = {"m": "momentum_buffer"} if kind == "sgd" else {"m": "exp_avg", "v": "exp_avg_sq"}
        for key, name in names.items():
            assert vw[name].data_ptr() == base + (lay[key][0] + o) * 4 and vw[name].shape == (n,)
        assert ("v" in lay) == (kind == "adam") and (core.v is None) == (kind == "sgd")
        if split:
            assert vw["master_residual"].data_ptr() == base + lay["lo"][0] * 4 + o * 2
            assert vw["master_residual"].dtype == torch.int16
        assert "max_exp_avg_sq" not in vw and "zero1_carry" not in core.views(o, n, (n,), ckpt=True)

    def rows_of(gbufs):
        so_ = np.asarray(offs, np.uint64)
        rows = np.zeros((len(SIZES), 9), np.uint64)
        rows[:, 0] = [g.data_ptr() + o * es for g, o in zip(gbufs, offs)]
        pp = np.uint64(P.data_ptr()) + so_ * np.uint64(es)
        if split:  # master = the bf16 param (in and out) + the int16 residual
            rows[:, 1], rows[:, 3] = pp, pp
            rows[:, 2] = np.uint64(core.lo.data_ptr()) + so_ * np.uint64(2)
        else:
            rows[:, 1], rows[:, 2] = pp, pp
        core.state_cols(rows, offs)
        rows[:, 8] = SIZES
        return rows

    built = []

    def new_set(rows):
        gz = _lib.ZS_BF16 if split else _lib.ZS_F32
        s = (SgdSet if kind == "sgd" else AdamSet)(rows, gz, _lib.ZS_BF16_SPLIT if split else _lib.ZS_BF16)
        built.append(s)
        return s

    def call(gbufs, counts):
        core.steps[:] = counts
        core.last_adam_bytes = 0
        return core.run_parts("t", rows_of(gbufs), np.arange(len(SIZES)), hparams_of, stream,
                              new_set=new_set)

    def check(what):
        torch.cuda.synchronize(gpu)
        for i, (o, n) in enumerate(zip(offs, SIZES)):
            got = {"param": P, "m": core.m, "v": core.v, "residual": core.lo, "vmax": core.vmax}
            want = {"param": ref.p, "m": ref.m, "v": ref.v if kind == "adam" else None,
                    "residual": ref.lo if split else None, "vmax": ref.vmax}
            for name, w in want.items():
                if w is not None:
                    assert _bits(got[name][o:o + n]).tobytes() == np.ascontiguousarray(w[i]).tobytes(), \
                        f"{what}: {name} of parameter {i}"

    # (b) one set per distinct (group, hp_key), each timed, their bytes summed
    nparts = len(set(zip(GROUP_OF, core.hp_key(COUNTS).tolist())))
    assert nparts == 3
    core.timing_events = []
    parts = call([G, G, G], COUNTS)
    ref.step(grads, COUNTS, hparams_of)
    assert len(parts) == len(built) == len(core.timing_events) == nparts
    assert sum(b for _, _, b in core.timing_events) == core.last_adam_bytes > 0
    assert sorted(g for g, _ in parts) == [0, 0, 1]

    # (c) the same call again: the cached sets themselves, nothing built, nothing retired
    again = call([G, G, G], COUNTS)
    ref.step(grads, COUNTS, hparams_of)
    assert all(a[1] is b[1] for a, b in zip(again, parts)) and len(built) == nparts
    assert not core.retired and len(core.timing_events) == 2 * nparts
    check("after two steps")  # (e)
    core.timing_events = None
    # one row's gradient elsewhere: its part's set is replaced, the old one kept until released
    moved = call([G, G2, G], COUNTS)
    ref.step([grads[0], grads2[1], grads[2]], COUNTS, hparams_of)
    assert len(built) == nparts + 1 and core.retired == [p[1] for p in parts if p[0] == 1]
    assert [m[1] is p[1] for m, p in zip(moved, parts)] == [p[0] != 1 for p in parts]
    assert core.n_retired() == 1
    check("after the moved gradient")
    core.release_retired()
    assert core.n_retired() == 0

    if kind == "adam":  # (d) amsgrad appears at a later step
        for g in opt.param_groups:
            g["amsgrad"] = True
        with pytest.raises(RuntimeError, match="amsgrad state buffer missing"):
            core.make_hp(hparams_of(0), 2)
        assert core.ensure_vmax() is core.vmax and core.vmax.shape == (L,)
        ref.vmax = [np.zeros(n, np.float32) for n in SIZES]
        for o, n in zip(offs, SIZES):
            vm = core.views(o, n, (n,))["max_exp_avg_sq"]
            assert vm.shape == (n,) and vm.data_ptr() == core.vmax.data_ptr() + o * 4
        assert core.views(offs[1], SIZES[1], (8, 8))["max_exp_avg_sq"].shape == (8, 8)
        counts = tuple(c + 1 for c in COUNTS)
        call([G, G, G], counts)  # (the rows gained the vmax column: every set is rebuilt)
        ref.step(grads, counts, hparams_of)
        assert core.n_retired() == nparts
        check("after the amsgrad step")
        core.release_retired()
