"""The constructor rules of ``accumulation_dtype`` (ZeRO-3 update mode), without a GPU: every
refusal comes before the world size is read, i.e. on every rank and before any collective."""
import inspect

import pytest
import torch


def _adam():
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))])


def test_only_none_and_float32_are_values():
    from zero_amd import zero3

    for bad in (torch.bfloat16, torch.float16, torch.float64, "float32", "fp32", 32, True):
        with pytest.raises(ValueError, match="accumulation_dtype must be None or torch.float32"):
            zero3.ShardedOptimizer(_adam(), update=True, grad_accumulation=True,
                                   accumulation_dtype=bad)


def test_needs_grad_accumulation():
    from zero_amd import zero3

    with pytest.raises(ValueError, match="grad_accumulation=True"):
        zero3.ShardedOptimizer(_adam(), update=True, accumulation_dtype=torch.float32)
    with pytest.raises(ValueError, match="grad_accumulation=True"):
        zero3.ShardedOptimizer(_adam(), accumulation_dtype=torch.float32)
    # reference mode with both: the older rule speaks first
    with pytest.raises(ValueError, match="update mode"):
        zero3.ShardedOptimizer(_adam(), grad_accumulation=True, accumulation_dtype=torch.float32)


def test_refusals_come_before_the_world_is_read(monkeypatch):
    from zero_amd import zero3

    def boom(*a, **k):
        raise AssertionError("the constructor read the world before refusing")

    monkeypatch.setattr(zero3, "get", boom)
    with pytest.raises(ValueError):
        zero3.ShardedOptimizer(_adam(), update=True, grad_accumulation=True,
                               accumulation_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        zero3.ShardedOptimizer(_adam(), update=True, accumulation_dtype=torch.float32)


def test_default_is_none_and_the_factory_passes_it_through():
    from zero_amd import zero3
    from zero_amd.training_utils import smollm3

    sig = inspect.signature(zero3.ShardedOptimizer.__init__)
    assert sig.parameters["accumulation_dtype"].default is None
    assert sig.parameters["accumulation_dtype"].kind is inspect.Parameter.KEYWORD_ONLY
    model = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="accumulation_dtype must be None or torch.float32"):
        smollm3.accumulating_optimizer(model, accumulation_dtype=torch.float16)
