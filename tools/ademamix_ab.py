"""In-process A/B of the fused AdEMAMix rule (csrc/zs_kernels.hip AdEMAMixRule) beside the instance
of Adam with amsgrad of the same encoding over the SAME buffers and segment rows: both stream m, v
and the vmax column (AdEMAMix: exp_avg_slow), so they move the same bytes.

ONE process, the same buffers, the two variants interleaved in every round after one untimed round,
every launch between two HIP events; per variant the median over the rounds and the spread
(max - min).  The yardstick is amsgrad Adam's own round-to-round spread.  Nothing is gated: the
figures are recorded side by side.  Encodings: "split" (bf16 gradient, split master), "bf16" (bf16
gradient, fp32 master beside its bf16 copy), "f32" (fp32 gradient, fp32 parameter in place).

Usage: python tools/ademamix_ab.py [--elems 268435456] [--rounds 9] [--out profiles/ademamix_ab.json]
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
    ap.add_argument("--elems", type=int, default=1 << 28)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from zero_amd import _lib
    from zero_amd.kernels import AdamSet, AdEMAMixSet, adam_hparams, ademamix_hparams

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream()
    n = args.elems // 4096 * 4096

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {"elems": n, "rounds": args.rounds, "encodings": {}}
    ahp = adam_hparams(1e-5, 0.9, 0.999, 1e-8, 0.01, 3, decoupled=True, amsgrad=True)
    mhp = ademamix_hparams(1e-5, 0.9, 0.999, 0.9999, 5.0, 1e-8, 0.01, 3)
    for enc in ("split", "bf16", "f32"):
        g32, split = enc == "f32", enc == "split"
        gen = torch.Generator(device=dev).manual_seed(0)
        g = torch.randn(n, device=dev, generator=gen) * 1e-3
        g = g if g32 else g.bfloat16()
        m = torch.randn(n, device=dev, generator=gen) * 0.02
        v = torch.rand(n, device=dev, generator=gen) * 1e-6
        x = torch.rand(n, device=dev, generator=gen) * 1e-6  # max_exp_avg_sq / exp_avg_slow
        if split:
            p = (torch.randn(n, device=dev, generator=gen) * 0.02).bfloat16()
            lo = torch.zeros(n, dtype=torch.int16, device=dev)
            row = [g.data_ptr(), p.data_ptr(), lo.data_ptr(), p.data_ptr()]
        else:
            p = torch.randn(n, device=dev, generator=gen) * 0.02
            pb = torch.zeros(n, dtype=torch.bfloat16, device=dev) if enc == "bf16" else None
            row = [g.data_ptr(), p.data_ptr(), p.data_ptr(), 0 if pb is None else pb.data_ptr()]
        rows = np.array([row + [m.data_ptr(), v.data_ptr(), x.data_ptr(), 0, n]], np.uint64)
        gz, pz = (_lib.ZS_F32 if g32 else _lib.ZS_BF16), (_lib.ZS_BF16_SPLIT if split else _lib.ZS_BF16)
        aset, mset = AdamSet(rows, gz, pz), AdEMAMixSet(rows, gz, pz)
        assert aset.bytes == mset.bytes
        variants = {"adam_amsgrad": lambda: aset.run(ahp, st), "ademamix": lambda: mset.run(mhp, st)}
        times = {k: [] for k in variants}
        for r in range(args.rounds + 1):  # interleaved; the first round is untimed
            for k, fn in variants.items():
                t = timed(fn)
                if r:
                    times[k].append(t)
        res = {k: {"ms": float(np.median(t)), "spread_ms": float(max(t) - min(t)),
                   "min_ms": float(min(t)), "max_ms": float(max(t)),
                   "gbps": mset.bytes / float(np.median(t)) / 1e6} for k, t in times.items()}
        res["bytes_per_elem"] = mset.bytes / n
        res["ademamix_over_adam_amsgrad"] = res["ademamix"]["ms"] / res["adam_amsgrad"]["ms"]
        res["adam_amsgrad_spread_rel"] = res["adam_amsgrad"]["spread_ms"] / res["adam_amsgrad"]["ms"]
        res["inside_adam_spread"] = bool(
            res["adam_amsgrad"]["min_ms"] <= res["ademamix"]["ms"] <= res["adam_amsgrad"]["max_ms"])
        out["encodings"][enc] = res
        print(json.dumps({enc: res}), flush=True)
        del aset, mset, g, m, v, x, p
        torch.cuda.synchronize()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
