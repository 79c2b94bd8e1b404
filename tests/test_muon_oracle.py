"""tests/_muon_oracle.py against torch's own bf16 Newton-Schulz on the CPU: equal where no product
is long enough for the accumulation order to flip a bf16 tie, within 0.01 normwise elsewhere; both
sit 0.011-0.016 from the unrounded iteration.

torch's side runs with oneDNN off, through ATen's own bf16 gemm, whose fp32 accumulation order is
the same on every AVX2 / AVX-512 CPU.  oneDNN picks its bf16 kernel by the CPU: with avx512_bf16 or
AMX it gives ATen's bits at these shapes, its AVX-512 kernel for CPUs without bf16 instructions
(``ONEDNN_MAX_CPU_ISA=AVX512_CORE`` shows it anywhere) flips one element of the (33, 70) case in
the first iterations, which the iteration carries to 0.0078 normwise."""
import numpy as np
import pytest
import torch
from torch.optim._muon import _zeropower_via_newtonschulz

import _muon_oracle as mo

SHAPES = [((1, 70), 0.0), ((33, 70), 0.0), ((96, 40), 0.0), ((64, 256), 0.01), ((128, 128), 0.01),
          ((256, 256), 0.01), ((130, 257), 0.01)]


@pytest.mark.parametrize("shape,bound", SHAPES)
def test_rounded_oracle_against_torch_bf16(shape, bound):
    g = torch.randn(shape, generator=torch.Generator().manual_seed(11))
    with torch.backends.mkldnn.flags(enabled=False):
        want = _zeropower_via_newtonschulz(g, mo.COEFFS, 5, 1e-7).double().numpy()
    got = mo.newton_schulz(g.double().numpy(), rounded=True)
    exact = mo.newton_schulz(g.double().numpy())
    dist = np.linalg.norm(got - want) / np.linalg.norm(want)
    far = [np.linalg.norm(x - exact) / np.linalg.norm(exact) for x in (got, want)]
    print(f"{shape}: rounded vs torch {dist:.4f}; from exact: rounded {far[0]:.4f}, torch {far[1]:.4f}")
    assert dist <= bound
    assert all(f <= 0.02 for f in far)
