"""In-process A/B of the fused LAMB (csrc/zs_lamb.hip) on the C4 parameter set, bf16 gradients over
the split master: pass L1 (zs_lambset_run_moments), the two per-parameter reduces plus the
finishing kernel, pass L2 (zs_lambset_run_apply) and, on the same buffers, the Adam stats instance
(zs_adamset_run_stats), whose step LAMB's is set beside (38 against 26 B/element).

ONE process, the same buffers, the settings interleaved in every round (the order reversed in
every other one) after one untimed round, every launch between two HIP events; per setting the
median of the rounds' medians and the spread between rounds (max - min).  Nothing is gated.

Usage: python tools/lamb_ab.py [--rounds 5] [--steps 10] [--out profiles/lamb_ab_c4.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))

PEAK_GBS = 8000.0  # MI355X HBM3E
BYTES = {"l1": 22, "l2": 16, "adam_stats": 26}  # per element, bf16 gradients, split master


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT
    from zero_amd._update import LambSetStage
    from zero_amd.kernels import AdamSet, adam_hparams, lamb_hparams
    from zero_amd.shapes import CONFIGS

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sizes = [int(np.prod(s)) for s in CONFIGS["C4"][1]()]
    off = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in sizes])]).astype(np.int64)
    N = int(off[-1])
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    w = torch.empty(N, dtype=torch.float32, device=dev).normal_(0.0, 0.02, generator=gen)
    T = {"hi": w.to(torch.bfloat16), "lo": torch.zeros(N, dtype=torch.int16, device=dev),
         "g": (torch.empty(N, dtype=torch.float32, device=dev).normal_(generator=gen) * 1e-3).to(
             torch.bfloat16),
         "m": torch.zeros(N, device=dev), "v": torch.zeros(N, device=dev)}
    del w
    at = lambda name, k: T[name].data_ptr() + int(off[k]) * T[name].element_size()  # noqa: E731
    rows = np.array([[at("g", k), at("hi", k), at("lo", k), at("hi", k), at("m", k), at("v", k), 0, 0, n]
                     for k, n in enumerate(sizes)], dtype=np.uint64)
    aset = AdamSet(rows, ZS_BF16, ZS_BF16_SPLIT)
    npar = len(sizes)
    stage = LambSetStage(aset, np.arange(npar), npar, 1e-3, dev)
    partials, neg_s, finish = stage.partials, stage.neg_s, lambda: stage.finish(st)
    hp, ahp = lamb_hparams(step=10), adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 10)
    st = torch.cuda.current_stream(dev)

    run = {"l1": lambda: aset.run_lamb_moments(hp, partials, st), "finish": finish,
           "l2": lambda: aset.run_lamb_apply(hp, neg_s, st),
           "adam_stats": lambda: aset.run_stats(ahp, partials, st)}
    settings = list(run)

    def block(name, n):
        ev = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            run[name]()
            e1.record(st)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    rounds = {s: [] for s in settings}
    for s in settings:  # one untimed round: code load, page tables, clocks
        block(s, args.steps)
    for r in range(args.rounds):
        for s in (settings if r % 2 == 0 else settings[::-1]):
            ms = block(s, args.steps)
            rounds[s].append(float(np.median(ms)))
            print(json.dumps({"round": r, "setting": s, "median_ms": rounds[s][-1],
                              "min_ms": min(ms), "max_ms": max(ms)}), flush=True)
    elems = int(sum(sizes))
    out = {"shard": "C4 " + CONFIGS["C4"][0], "elems": elems, "segments": npar,
           "rounds": args.rounds, "steps_per_round": args.steps, "settings": {}}
    for s in settings:
        med = float(np.median(rounds[s]))
        out["settings"][s] = {"round_medians_ms": rounds[s], "median_ms": med,
                              "spread_ms": max(rounds[s]) - min(rounds[s])}
        if s in BYTES:
            gbs = BYTES[s] * elems / med / 1e6
            out["settings"][s].update(bytes_per_elem=BYTES[s], gbs=gbs, of_peak=gbs / PEAK_GBS)
    S = out["settings"]
    step = S["l1"]["median_ms"] + S["finish"]["median_ms"] + S["l2"]["median_ms"]
    out["lamb_step_ms"] = step
    out["vs_adam_stats"] = {"ratio": step / S["adam_stats"]["median_ms"], "byte_ratio": 38 / 26,
                            "excess_ms": step - 38 / 26 * S["adam_stats"]["median_ms"],
                            "adam_spread_ms": S["adam_stats"]["spread_ms"]}
    r = stage.ratios.cpu().numpy()
    out["sane"] = bool(np.isfinite(r).all() and (r > 0).all())
    print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
