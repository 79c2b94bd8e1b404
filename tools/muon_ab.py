"""In-process A/B of the fused Muon (csrc/zs_muon.hip) at the 2-D decoder shapes of C4 (the embedding
excluded): each of the three Newton-Schulz products beside ``torch.mm`` / ``torch.addmm`` (hipBLASLt)
on the same operands, the whole fused step beside ``torch.optim.Muon.step()`` on the device over
the same matrices, and the stream passes M1, M2 and P in GB/s.

ONE process, the same buffers, the variants interleaved in every round after one untimed round,
every launch between two HIP events; per variant the median over the rounds and the spread
(max - min).  Nothing is gated: the figures are recorded side by side.  ``--layers`` decoder layers
of matrices take part in the whole step (7 matrices a layer).

Usage: python tools/muon_ab.py [--rounds 5] [--layers 4] [--out profiles/muon_ab_c4.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from zero_amd import _lib
    from zero_amd.kernels import MuonSet, muon_gemm_nt, muon_hparams
    from zero_amd.shapes import decoder_shapes

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    shapes = [s for s in decoder_shapes("C4", args.layers)[1:] if len(s) == 2]
    a, b, c = 3.4445, -4.7750, 2.0315

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def ab(variants):
        """{name: fn} -> {name: (median ms, spread ms)}, interleaved rounds after an untimed one."""
        times = {k: [] for k in variants}
        for r in range(args.rounds + 1):
            for k, fn in variants.items():
                t = timed(fn)
                if r:
                    times[k].append(t)
        return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in times.items()}

    out = {"config": "C4 decoder matrices", "layers": args.layers, "rounds": args.rounds, "products": []}
    gen = torch.Generator(device=dev).manual_seed(0)
    for R, C in sorted(set(shapes)):
        r, cc = min(R, C), max(R, C)
        X = (torch.randn(r, cc, device=dev, generator=gen) / cc ** 0.5).bfloat16()
        XT = X.T.contiguous()
        A, Bm, Xn, XTn = (torch.empty(s, dtype=torch.bfloat16, device=dev)
                          for s in ((r, r), (r, r), (r, cc), (cc, r)))
        muon_gemm_nt(X, X, A, sym=True, stream=st)
        muon_gemm_nt(A, A, Bm, E=A, alpha=c, beta=b, sym=True, stream=st)
        flops = {"gram": 2 * r * r * cc, "poly": 2 * r * r * r, "apply": 2 * r * r * cc}
        res = ab({
            "gram": lambda: muon_gemm_nt(X, X, A, sym=True, stream=st),
            "gram_full": lambda: muon_gemm_nt(X, X, A, D2=None, stream=st),
            "gram_torch": lambda: torch.mm(X, X.T),
            "poly": lambda: muon_gemm_nt(A, A, Bm, E=A, alpha=c, beta=b, sym=True, stream=st),
            "poly_torch": lambda: torch.addmm(A, A, A, beta=b, alpha=c),
            "apply": lambda: muon_gemm_nt(Bm, XT, Xn, E=X, D2=XTn, beta=a, stream=st),
            "apply_torch": lambda: torch.addmm(X, Bm, X, beta=a),
        })
        row = {"r": r, "c": cc}
        for k, (ms, spread) in res.items():
            row[k] = {"ms": ms, "spread_ms": spread, "tflops": flops[k.split("_")[0]] / ms / 1e9}
        out["products"].append(row)
        print(json.dumps(row), flush=True)

    # the whole step and its stream passes over `layers` layers of matrices, fp32 master in place
    ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.02) for s in shapes]
    gs = [torch.randn(s, device=dev, generator=gen) * 1e-3 for s in shapes]
    bufs = [torch.zeros(s, device=dev) for s in shapes]
    rows = np.array([[g.data_ptr(), p.data_ptr(), p.data_ptr(), 0, m.data_ptr(), *p.shape, i]
                     for i, (p, g, m) in enumerate(zip(ps, gs, bufs))], np.uint64)
    mset, hp = MuonSet(rows, _lib.ZS_F32, _lib.ZS_BF16), muon_hparams(lr=1e-3)
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for q, g in zip(qs, gs):
        q.grad = g
    ref = torch.optim.Muon(qs, lr=1e-3)
    res = ab({"fused_step": lambda: mset.run(hp, st), "torch_step": ref.step,
              "m1": lambda: mset.run_pass(hp, 0, st), "m2": lambda: mset.run_pass(hp, 1, st),
              "products": lambda: mset.run_pass(hp, 2, st), "p": lambda: mset.run_pass(hp, 3, st)})
    nbytes = {"m1": mset.m1_bytes, "m2": mset.m2_bytes, "p": mset.p_bytes}
    out["step"] = {k: {"ms": ms, "spread_ms": sp, **({"gbps": nbytes[k] / ms / 1e6} if k in nbytes else {})}
                   for k, (ms, sp) in res.items()}
    out["step"]["matrices"] = len(shapes)
    out["step"]["scratch_bytes"], out["step"]["batches"] = mset.scratch_bytes, mset.batches
    out["step"]["flops_nominal"] = 5 * mset.flops_iter
    out["step"]["flops_run"] = 5 * mset.flops_iter_run
    out["step"]["products_tflops_nominal"] = 5 * mset.flops_iter / out["step"]["products"]["ms"] / 1e9
    print(json.dumps(out["step"]), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
