"""Per-parameter update and weight norms, the host side without a GPU: every refusal through the
``check_*`` functions and through the optimizers' constructors (before any device work), the slot
rule restated in numpy (``slot_counts``, which tests/test_gpu_update_norms_kernel.py holds the
library to) against counts worked out by hand, and the CSR of slot ranges with the ``touched`` mask
(``UpdateNorms.tables``) for a parameter cut across two sets and for parameters without a range."""
import numpy as np
import pytest
import torch

CHUNKS = (2048, 4096)


def slot_counts(C, segs, shifted=()):
    """include/zero_amd.h zs_adamset_update_norm_slots, restated: the slots per plane of every
    segment (offset, n, has_grad) -- 4 per chunk of C elements of its vector part (the 4-aligned
    prefix of an aligned segment), then 4 per 256-element chunk of its scalar part."""
    out = []
    for k, (_, n, _) in enumerate(segs):
        nv = 0 if k in shifted else n & ~3
        out.append(4 * -(-nv // C) + 4 * -(-(n - nv) // 256))
    return np.array(out, np.int64)


@pytest.mark.parametrize("C", CHUNKS)
def test_slot_rule(C):
    lengths = [0, 1, 3, 4, 255, 1024, C - 4, C, C + 4, 3 * C + 1028]
    segs = [(0, n, True) for n in lengths]
    #        0  1  3  4  255    1024  C-4  C  C+4    3C+1028 (4 chunks)
    want = [0, 4, 4, 4, 4 + 4, 4,    4,   4, 4 + 4, 16]
    assert list(slot_counts(C, segs)) == want
    # unaligned: everything in 256-element chunks
    un = [0, 4, 4, 4, 4, 16, 4 * ((C - 4 + 255) // 256), 4 * (C // 256), 4 * (C // 256 + 1),
          4 * ((3 * C + 1028 + 255) // 256)]
    assert list(slot_counts(C, segs, shifted=range(len(segs)))) == un
    assert un[6:9] == ([32, 32, 36] if C == 2048 else [64, 64, 68])
    # a segment without a gradient has the slots of one with (it is updated like any other)
    assert list(slot_counts(C, [(0, C + 4, False)])) == [8]


def test_check_update_norms():
    from zero_amd._update import check_update_norms, check_update_norms_group

    check_update_norms("adam", False)
    check_update_norms("adam", False, torch.float32, "split")
    check_update_norms("adam", False, None, "fp32")
    for args, kw, text in ((("sgd", False), {}, "torch.optim.SGD"),
                           (("adam", False, torch.bfloat16), {}, "state_dtype=torch.bfloat16"),
                           (("adam", False, None, "none"), {}, "master='none'"),
                           (("adam", False), dict(ema=True), "ema_decay"),
                           (("adam", True), {}, "ZeRO-1 at world size > 1")):
        with pytest.raises(ValueError, match=f"param_update_norms is not supported with .*{text}"):
            check_update_norms(*args, **kw)
    check_update_norms_group({"amsgrad": False})
    with pytest.raises(ValueError, match="param_update_norms is not supported with amsgrad"):
        check_update_norms_group({"amsgrad": True})


def _adam(**kw):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(8))], lr=1e-3, **kw)


def _bf16_adam(**kw):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))], lr=1e-3, **kw)


def _sgd():
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(8))], lr=1e-3, momentum=0.9)


REFUSED = (  # (optimizer, keywords, message): what every engine refuses alike
    (_sgd, {}, "SGD"),
    (lambda: _adam(amsgrad=True), {}, "param_update_norms.*amsgrad"),
    (lambda: _bf16_adam(betas=(0.9, 0.99)), dict(state_dtype=torch.bfloat16),
     "param_update_norms.*bfloat16"),
    (_bf16_adam, dict(master="none"), "param_update_norms.*master='none'"),
    (_adam, dict(ema_decay=0.9), "param_update_norms.*ema_decay"),
)


def test_zero2_constructor_refuses_before_any_device_work():
    """CPU parameters, no process group: each error below comes before the first thing that would
    need either."""
    from zero_amd import zero2

    for make, kw, text in REFUSED:
        with pytest.raises(ValueError, match=text):
            zero2.ShardedOptimizer(make(), param_update_norms=True, **kw)
    with pytest.raises(ValueError, match="param_update_norms.*bucket arena"):
        zero2.ShardedOptimizer(_adam(), param_update_norms=True, arena="buckets")
    with pytest.raises(ValueError, match="param_update_norms.*overlap"):
        zero2.ShardedOptimizer(_adam(), param_update_norms=True, overlap=True)


def test_zero1_constructor_refuses_before_any_device_work(monkeypatch):
    """ZeRO-1 asks for the world size first (its carry): answered here without a process group."""
    from zero_amd import _sharded, zero1

    world = {"ws": 2, "rank": 0}
    monkeypatch.setattr(_sharded, "get", lambda what, dm=None: world[what])
    with pytest.raises(ValueError, match="param_update_norms.*ZeRO-1 at world size > 1"):
        zero1.ShardedOptimizer(_adam(), param_update_norms=True)
    world["ws"] = 1
    for make, kw, text in REFUSED:
        with pytest.raises(ValueError, match=text):
            zero1.ShardedOptimizer(make(), param_update_norms=True, **kw)
    with pytest.raises(ValueError, match="param_update_norms.*bucket arena"):
        zero1.ShardedOptimizer(_adam(), param_update_norms=True, layout="flat")  # (the bucket arena)
    with pytest.raises(ValueError, match="param_update_norms.*overlap"):
        zero1.ShardedOptimizer(_adam(), param_update_norms=True, overlap=True)


def test_zero3_constructor_refuses_before_any_device_work():
    from zero_amd import zero3

    with pytest.raises(ValueError, match="param_update_norms.*update mode"):
        zero3.ShardedOptimizer(_adam(), update=False, param_update_norms=True)
    for make, kw, text in REFUSED:
        with pytest.raises(ValueError, match=text):
            zero3.ShardedOptimizer(make(), update=True, param_update_norms=True, **kw)


def test_a_core_refuses_amsgrad_that_appears_later():
    """A group that turns amsgrad on between steps: refused where the core would allocate the
    buffer and where it makes the launch's hyper-parameters."""
    from zero_amd._update import UpdateCore

    core = UpdateCore.__new__(UpdateCore)
    core.update_norms = True
    with pytest.raises(ValueError, match="param_update_norms.*amsgrad"):
        core.ensure_vmax()
    assert UpdateCore.update_norms is False  # the switch is off unless the constructor sets it


def test_csr_and_touched_mask():
    """Two sets collected in order.  Set 0 (12 slots per plane, planes at 0 and 12) has rows for
    parameters 0 (8 slots), 2 (a row without slots) and 1 (4 slots); set 1 (20 slots, planes at 24
    and 44) for parameters 0 (16 slots) and 3 (4 slots).  Parameter 0 is cut across both sets, in
    the order they were collected; parameters 2 and 4 have no range and are not touched."""
    from zero_amd._update import UpdateNorms, slot_csr

    offs = [np.array([0, 8, 8, 12], np.int64), np.array([0, 16, 20], np.int64)]
    pars = [np.array([0, 2, 1]), np.array([0, 3])]
    base = np.array([0, 24], np.int64)  # each set owns two planes of its slot count
    csr, touched = UpdateNorms.tables(base, offs, pars, 5)
    assert csr.dtype == np.int64 and touched.dtype == np.float32
    n, nr = 5, 4
    assert len(csr) == n + 1 + 3 * nr
    assert list(csr[:n + 1]) == [0, 2, 3, 3, 4, 4]                 # row_ptr
    assert list(csr[n + 1:n + 1 + nr]) == [0, 24, 8, 40]           # the update plane's ranges
    assert list(csr[n + 1 + nr:n + 1 + 2 * nr]) == [12, 44, 20, 60]  # the weight plane's
    assert list(csr[n + 1 + 2 * nr:]) == [8, 16, 4, 4]             # slots per range
    assert list(touched) == [1.0, 1.0, 0.0, 1.0, 0.0]
    # the shared builder: what GradClip's CSR is made of
    row_ptr, lo, cnt = slot_csr(base, offs, pars, 5)
    assert list(row_ptr) == [0, 2, 3, 3, 4, 4] and list(lo) == [0, 24, 8, 40] and list(cnt) == [8, 16, 4, 4]
    # nothing collected: every row empty, nothing touched
    csr, touched = UpdateNorms.tables(np.zeros(0, np.int64), [], [], 3)
    assert list(csr) == [0, 0, 0, 0] and list(touched) == [0.0, 0.0, 0.0]
