"""In-process A/B of the fused Schedule-Free AdamW rule (csrc/zs_kernels.hip SfAdamRule) beside the
Adam rule's instance of the same encoding over the SAME buffers and segment rows, and the swap
kernel's rate in each of its forms.

ONE process, the same buffers, the variants interleaved in every round after one untimed round,
every launch between two HIP events; per variant the median over the rounds and the spread
(max - min).  The yardstick is Adam's own round-to-round spread: the new rule moves the same bytes.
Nothing is gated: the figures are recorded side by side.  Encodings: "split" (bf16 gradient, split
master), "bf16" (bf16 gradient, fp32 master beside its bf16 copy), "f32" (fp32 gradient, fp32
parameter in place).

Usage: python tools/sfadam_ab.py [--elems 268435456] [--rounds 9] [--out profiles/sfadam_ab.json]
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
    from zero_amd.kernels import AdamSet, SfAdamSet, adam_hparams, sfadam_hparams

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

    def ab(variants):
        """{name: (fn, bytes)} -> {name: {ms, spread_ms, gbps}}, interleaved rounds after an
        untimed one."""
        times = {k: [] for k in variants}
        for r in range(args.rounds + 1):
            for k, (fn, _) in variants.items():
                t = timed(fn)
                if r:
                    times[k].append(t)
        return {k: {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)),
                    "min_ms": float(min(v)), "max_ms": float(max(v)),
                    "gbps": variants[k][1] / float(np.median(v)) / 1e6} for k, v in times.items()}

    out = {"elems": n, "rounds": args.rounds, "encodings": {}}
    ahp = adam_hparams(1e-5, 0.9, 0.999, 1e-8, 0.01, 3, decoupled=True)
    shp = sfadam_hparams(1e-5, 0.9, 0.999, 1e-8, 0.01, 3, 1.0 / 3.0)
    b1 = 0.9
    for enc in ("split", "bf16", "f32"):
        g32, split = enc == "f32", enc == "split"
        gen = torch.Generator(device=dev).manual_seed(0)
        g = torch.randn(n, device=dev, generator=gen) * 1e-3
        g = g if g32 else g.bfloat16()
        m = torch.randn(n, device=dev, generator=gen) * 0.02
        v = torch.rand(n, device=dev, generator=gen) * 1e-6
        if split:
            p = (torch.randn(n, device=dev, generator=gen) * 0.02).bfloat16()
            lo = torch.zeros(n, dtype=torch.int16, device=dev)
            row = [g.data_ptr(), p.data_ptr(), lo.data_ptr(), p.data_ptr()]
        else:
            p = torch.randn(n, device=dev, generator=gen) * 0.02
            pb = torch.zeros(n, dtype=torch.bfloat16, device=dev) if enc == "bf16" else None
            row = [g.data_ptr(), p.data_ptr(), p.data_ptr(), 0 if pb is None else pb.data_ptr()]
        rows = np.array([row + [m.data_ptr(), v.data_ptr(), 0, 0, n]], np.uint64)
        gz, pz = (_lib.ZS_F32 if g32 else _lib.ZS_BF16), (_lib.ZS_BF16_SPLIT if split else _lib.ZS_BF16)
        aset, sset = AdamSet(rows, gz, pz), SfAdamSet(rows, gz, pz)
        assert aset.bytes == sset.bytes
        res = ab({"adam": (lambda: aset.run(ahp, st), aset.bytes),
                  "sfadam": (lambda: sset.run(shp, st), sset.bytes)})
        # the swap: in place (12 B/element) or, beside an fp32 master, the copy alone (10 and 6)
        ev, tr = (10 * n, 6 * n) if enc == "bf16" else (12 * n, 12 * n)
        res.update(ab({"swap_eval": (lambda: sset.swap(1 - 1 / b1, True, st), ev),
                       "swap_train": (lambda: sset.swap(1 - b1, False, st), tr)}))
        res["bytes_per_elem"] = sset.bytes / n
        res["sfadam_over_adam"] = res["sfadam"]["ms"] / res["adam"]["ms"]
        res["inside_adam_spread"] = bool(res["adam"]["min_ms"] <= res["sfadam"]["ms"] <= res["adam"]["max_ms"])
        out["encodings"][enc] = res
        print(json.dumps({enc: res}), flush=True)
        del aset, sset, g, m, v, p
        torch.cuda.synchronize()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
