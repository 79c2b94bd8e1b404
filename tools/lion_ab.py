"""In-process A/B of the fused Lion update against fused SGD-with-momentum and fused Adam, on the
split master at a benchmark configuration's size (default C4).

Placement differs from process to process, so the variants are judged here: ONE process, the same
placed buffers (bf16 parameter, int16 residual, bf16 gradient, one fp32 array each for m and v; the
bf16 moments live in the first half of the same arrays), one kernel set per variant over the same
segments, stepped in alternating blocks.  Every launch is timed with HIP events around it.  One
untimed round comes first.  Per variant: the median of each round, their median and the spread
(max - min) between rounds.

The gate: Lion with fp32 momentum moves SGD-with-momentum's bytes (18 B/element) through the same
skeleton, so its median may exceed the SGD variant's by at most twice the SGD variant's own spread
in this run.  The bf16-momentum variants (14 B/element) have no gate; their ratio to the
fp32-momentum variant is recorded beside Adam's 26 -> 18 B ratio from the same run.

Usage: python tools/lion_ab.py [--rounds 7] [--steps 30] [--config C4] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))

VARIANTS = ("lion_f32", "lion_bf16", "lion_bf16_sr", "sgd_mom", "adam_f32", "adam_bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--config", default="C4", choices=["C2", "C3", "C4", "C5"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"

    import numpy as np
    import torch

    from zero_amd import _lib
    from zero_amd.kernels import (AdamSet, LionSet, SgdSet, adam_hparams, lion_hparams, sgd_hparams,
                                  sr_keys)
    from zero_amd.shapes import CONFIGS

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    name, shape_fn = CONFIGS[args.config]
    numels = [int(np.prod(s, dtype=np.int64)) for s in shape_fn()]
    offs, total = [], 0
    for n in numels:  # every segment 256-byte aligned in every array
        offs.append(total)
        total += (n + 127) // 128 * 128
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    hi = torch.empty(total, dtype=torch.float32, device=dev).normal_(0.0, 0.02, generator=gen).to(
        torch.bfloat16)
    lo = torch.zeros(total, dtype=torch.int16, device=dev)
    g = (torch.empty(total, dtype=torch.float32, device=dev).normal_(generator=gen) * 1e-3).to(
        torch.bfloat16)
    m = torch.zeros(total, dtype=torch.float32, device=dev)
    v = torch.zeros(total, dtype=torch.float32, device=dev)

    def rows(ssz, with_v):
        r = np.zeros((len(numels), 9), np.uint64)
        o = np.asarray(offs, np.uint64)
        r[:, 0] = np.uint64(g.data_ptr()) + o * np.uint64(2)
        r[:, 1] = r[:, 3] = np.uint64(hi.data_ptr()) + o * np.uint64(2)
        r[:, 2] = np.uint64(lo.data_ptr()) + o * np.uint64(2)
        r[:, 4] = np.uint64(m.data_ptr()) + o * np.uint64(ssz)
        if with_v:
            r[:, 5] = np.uint64(v.data_ptr()) + o * np.uint64(ssz)
        r[:, 8] = np.asarray(numels, np.uint64)
        return r

    BF16, SPLIT, F32 = _lib.ZS_BF16, _lib.ZS_BF16_SPLIT, _lib.ZS_F32
    sets = {
        "lion_f32": LionSet(rows(4, False), BF16, SPLIT),
        "lion_bf16": LionSet(rows(2, False), BF16, SPLIT, state_dtype=BF16),
        "lion_bf16_sr": LionSet(rows(2, False), BF16, SPLIT, state_dtype=BF16,
                                state_rounding="stochastic"),
        "sgd_mom": SgdSet(rows(4, False), BF16, SPLIT),
        "adam_f32": AdamSet(rows(4, True), BF16, SPLIT),
        "adam_bf16": AdamSet(rows(2, True), BF16, SPLIT, state_dtype=BF16),
    }
    lhp = lion_hparams(1e-4, 0.9, 0.99, 0.1)
    shp = sgd_hparams(1e-3, 0.9)
    st = torch.cuda.current_stream()
    count = {k: 0 for k in VARIANTS}

    def launch(k):
        count[k] += 1
        if k == "lion_bf16_sr":
            sets[k].run(lhp, st, sr=(m.data_ptr(), sr_keys(0, count[k])))
        elif k.startswith("lion"):
            sets[k].run(lhp, st)
        elif k == "sgd_mom":
            sets[k].run(shp, st)
        else:  # (beta2 0.99: within the bound of bf16 moments rounded to nearest)
            sets[k].run(adam_hparams(1e-3, 0.9, 0.99, 1e-8, 0.0, count[k]), st)

    def block(k, n):
        ev = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            launch(k)
            e1.record(st)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    def reset():  # a variant starts from zeroed state: the fp32 and bf16 views share the arrays
        m.zero_()
        v.zero_()

    rounds = {k: [] for k in VARIANTS}
    for k in VARIANTS:  # one untimed round: code load, page tables, clocks
        reset()
        block(k, args.steps)
    for r in range(args.rounds):
        for k in (VARIANTS if r % 2 == 0 else VARIANTS[::-1]):
            reset()
            ms = block(k, args.steps)
            rounds[k].append(float(np.median(ms)))
            print(json.dumps({"round": r, "variant": k, "median_ms": rounds[k][-1], "min_ms": min(ms),
                              "max_ms": max(ms)}), flush=True)
    elems = int(sum(numels))
    summary = {"config": f"{args.config} {name}", "params": elems, "master": "split",
               "rounds": args.rounds, "steps_per_round": args.steps, "variants": {}}
    for k in VARIANTS:
        med = float(np.median(rounds[k]))
        summary["variants"][k] = {"round_medians_ms": rounds[k], "median_ms": med,
                                  "spread_ms": max(rounds[k]) - min(rounds[k]),
                                  "bytes_per_element": sets[k].bytes / elems,
                                  "gbs": sets[k].bytes / med / 1e6}
    vs = summary["variants"]
    margin = 2.0 * vs["sgd_mom"]["spread_ms"]
    over = vs["lion_f32"]["median_ms"] - vs["sgd_mom"]["median_ms"]
    summary["gate"] = {"lion_f32_minus_sgd_mom_ms": over, "two_sgd_spreads_ms": margin,
                       "met": bool(over <= margin)}
    summary["ratios"] = {
        "lion_bf16_over_lion_f32": vs["lion_bf16"]["median_ms"] / vs["lion_f32"]["median_ms"],
        "lion_bf16_sr_over_lion_f32": vs["lion_bf16_sr"]["median_ms"] / vs["lion_f32"]["median_ms"],
        "adam_bf16_over_adam_f32": vs["adam_bf16"]["median_ms"] / vs["adam_f32"]["median_ms"],
        "bytes_14_over_18": 14 / 18, "bytes_18_over_26": 18 / 26}
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
