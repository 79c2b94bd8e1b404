"""In-process A/B of the fused NorMuon passes (csrc/zs_muon.hip) at the 2-D decoder shapes of C4 (the
embedding excluded), on one MuonSet with row state over ``--layers`` decoder layers of matrices
(7 a layer, fp32 master in place): N1, N2 and N3 in ms and GB/s, Muon's element-addressed P on the
same matrices beside the row-tiled N3 (they move the same bytes), and the whole NorMuon step beside
the whole Muon step (the difference is the cost of the normalisation).

ONE process, the same buffers, the variants interleaved in every round after one untimed round,
every launch between two HIP events; per variant the median over the rounds and the spread
(max - min).  Nothing is gated: the figures are recorded side by side.

Usage: python tools/normuon_ab.py [--rounds 5] [--layers 4] [--out profiles/normuon_ab_c4.json]
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
    from zero_amd.kernels import MuonSet, muon_hparams, normuon_hparams
    from zero_amd.shapes import decoder_shapes

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    shapes = [s for s in decoder_shapes("C4", args.layers)[1:] if len(s) == 2]
    gen = torch.Generator(device=dev).manual_seed(0)
    ps = [torch.randn(s, device=dev, generator=gen) * 0.02 for s in shapes]
    gs = [torch.randn(s, device=dev, generator=gen) * 1e-3 for s in shapes]
    bufs = [torch.zeros(s, device=dev) for s in shapes]
    vs = [torch.zeros(s[0], device=dev) for s in shapes]
    rows = np.array([[g.data_ptr(), p.data_ptr(), p.data_ptr(), 0, m.data_ptr(), *p.shape, i]
                     for i, (p, g, m) in enumerate(zip(ps, gs, bufs))], np.uint64)
    mset = MuonSet(rows, _lib.ZS_F32, _lib.ZS_BF16)
    mset.attach_rows([v.data_ptr() for v in vs])
    hm, hn = muon_hparams(lr=1e-3), normuon_hparams(lr=1e-3)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    variants = {"normuon_step": lambda: mset.run_normuon(hn, st), "muon_step": lambda: mset.run(hm, st),
                "n1": lambda: mset.run_normuon_pass(hn, 3, st), "n2": lambda: mset.run_normuon_pass(hn, 4, st),
                "n3": lambda: mset.run_normuon_pass(hn, 5, st), "muon_p": lambda: mset.run_pass(hm, 3, st)}
    times = {k: [] for k in variants}
    for r in range(args.rounds + 1):  # (round 0 untimed)
        for k, fn in variants.items():
            t = timed(fn)
            if r:
                times[k].append(t)
    nrow = sum(s[0] for s in shapes)
    nbytes = {"n1": 2 * mset.elems + 8 * nrow, "n2": 20 * nrow, "n3": mset.p_bytes + 4 * nrow,
              "muon_p": mset.p_bytes}
    out = {"config": "C4 decoder matrices", "layers": args.layers, "rounds": args.rounds,
           "matrices": len(shapes), "rows": nrow, "elems": mset.elems, "batches": mset.batches,
           "scratch_bytes": mset.scratch_bytes}
    for k, v in times.items():
        ms = float(np.median(v))
        out[k] = {"ms": ms, "spread_ms": float(max(v) - min(v)),
                  **({"bytes": nbytes[k], "gbps": nbytes[k] / ms / 1e6} if k in nbytes else {})}
    out["normalisation_ms"] = out["normuon_step"]["ms"] - out["muon_step"]["ms"]
    print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
