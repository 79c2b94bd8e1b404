"""Host logic of the shared update core (zero_amd/_update.py) that needs no GPU: the flat state
layout, the step key of the hyper-parameter struct, the owner ranges and the group
hyper-parameter pick."""
import itertools

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("L", [0, 1, 2, 63, 4099])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_state_layout(kind, L):
    from zero_amd._update import state_layout

    for split, fp32_master, carry, momentum in itertools.product((False, True), repeat=4):
        total, lay = state_layout(kind, L, split=split, fp32_master=fp32_master, carry=carry,
                                  momentum=momentum)
        nmom = 2 if kind == "adam" else int(momentum)
        nf = nmom + carry + fp32_master
        assert total == nf * L + (L + 1) // 2 * split
        # which arrays exist: SGD has no v, and no m without momentum
        assert ("m" in lay) == (nmom >= 1) and ("v" in lay) == (kind == "adam")
        assert ("carry" in lay) == carry and ("master" in lay) == fp32_master
        assert ("lo" in lay) == split
        # in the order m, v, carry, master, lo, back to back: no gap, no overlap
        order = [n for n in ("m", "v", "carry", "master", "lo") if n in lay]
        assert list(lay) == order
        end = 0
        for name in order:
            off, dt = lay[name]
            assert off == end, (name, lay)
            assert dt == (torch.int16 if name == "lo" else torch.float32)
            end = off + ((L + 1) // 2 if name == "lo" else L)
        assert end == total


def test_hp_key():
    from zero_amd._update import UpdateCore

    steps = [0, 1, 1, 2, 7]
    for kind, want in (("adam", [0, 1, 1, 2, 7]), ("sgd", [0, 1, 1, 0, 0])):
        core = UpdateCore.__new__(UpdateCore)  # (hp_key reads the kind alone: no device needed)
        core.kind = kind
        key = core.hp_key(steps)
        assert key.dtype == np.int64 and key.tolist() == want


def test_owner_range():
    from zero_amd._update import owner_range

    for n in range(41):
        for ws in range(1, 10):
            ends = []
            for rank in range(ws):
                per, rem = n // ws, n % ws  # zero1.py:55-62, the arithmetic it replaces
                start = rank * per + min(rank, rem)
                end = start + per + (1 if rank < rem else 0)
                assert owner_range(n, ws, rank) == (start, end)
                ends.append((start, end))
            assert ends[0][0] == 0 and ends[-1][1] == n  # the ranges tile 0..n
            assert all(a[1] == b[0] for a, b in zip(ends, ends[1:]))


def test_group_hparams():
    from zero_amd._sharded import adam_group_hparams, group_hparams, sgd_group_hparams

    p = [torch.nn.Parameter(torch.zeros(2))]
    adam = torch.optim.Adam(p, lr=2e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, amsgrad=True)
    adamw = torch.optim.AdamW(p, lr=torch.tensor(1e-3), weight_decay=0.01)
    sgd = torch.optim.SGD(p, lr=0.1, momentum=0.9, dampening=0.1, weight_decay=0.01, maximize=True)
    for opt in (adam, adamw):
        g = opt.param_groups[0]
        h = group_hparams("adam", g, opt)
        assert h == adam_group_hparams(g, opt)
        assert h["decoupled"] is (opt is adamw) and h["amsgrad"] is (opt is adam)
    h = group_hparams("adam", adam.param_groups[0], adam)
    assert h == dict(lr=2e-3, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=0.1, amsgrad=True,
                     maximize=False, decoupled=False)
    assert group_hparams("adam", adamw.param_groups[0], adamw)["lr"] == pytest.approx(1e-3, rel=1e-6)
    g = sgd.param_groups[0]
    h = group_hparams("sgd", g, sgd)
    assert h == sgd_group_hparams(g) == dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=0.01,
                                             nesterov=False, maximize=True, amsgrad=False)
    with pytest.raises(ValueError, match="differentiable"):
        group_hparams("sgd", dict(g, differentiable=True), sgd)
