"""What ZeRO-3 gradient accumulation checks without a GPU: the constructor refuses the flag in
reference mode, and the inputs of tests/test_gpu_zero3_accumulate.py do make accumulation inexact."""
import pytest
import torch

import _accum_inputs as ai


def test_reference_mode_refuses_the_flag():
    from zero_amd import zero3

    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="update mode"):
        zero3.ShardedOptimizer(torch.optim.Adam(p), grad_accumulation=True)
    with pytest.raises(ValueError, match="update mode"):
        zero3.ShardedOptimizer(torch.optim.SGD(p, lr=0.1), update=False, grad_accumulation=True)


@pytest.mark.parametrize("arena", ["f32", "bf16"])
def test_inputs_make_accumulation_inexact(arena):
    for ws in (1, 2, 3):
        total, inexact, ties = ai.addition_stats(ws, arena, arena)
        assert total > 3000 and 4 * inexact >= total and ties > 0


def test_schedule_has_the_skips():
    on = [[[ai.active(s, p, m) for m in range(len(ai.SHAPES))] for p in range(ai.PASSES)]
          for s in range(ai.STEPS)]
    assert all(not on[s][1][1] for s in range(ai.STEPS))
    assert all(not on[1][p][2] for p in range(ai.PASSES))
    assert sum(not x for s in on for p in s for x in p) == 3 + 3
    for ws in (2, 3):
        _, had = ai.accumulated(1, ai.PASSES - 1, 2, ws, "f32", "f32")
        assert not had
