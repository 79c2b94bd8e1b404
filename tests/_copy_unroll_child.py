"""Child of test_gpu_stream_edges.test_copy_edges_other_unrolls: the chunk-edge copy case at the
chunk K given on the command line, in a process whose environment selects the copy set's unroll
before the library reads it.  Exits non-zero on a mismatch."""
import os
import sys
from pathlib import Path

TESTS = Path(__file__).resolve().parent
REPO = TESTS.parent
for p in (str(REPO), str(REPO / "distributed-training-sandbox_amd"), str(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch

    import test_gpu_stream_edges as edges

    K = int(sys.argv[1])
    assert K == 4096 * int(os.environ[edges.COPY_UNROLL_ENV]), "K is not the chunk of the unroll asked for"
    assert torch.cuda.is_available(), "no GPU visible"
    gpu = torch.device("cuda:0")
    for nt in (-1, 1):
        edges.copy_edges_case(gpu, K, nt, "set")  # raises on a mismatch
    print(f"copy edges ok K={K}")


if __name__ == "__main__":
    main()
