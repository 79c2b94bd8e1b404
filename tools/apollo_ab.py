"""In-process A/B of the fused APOLLO (csrc/zs_apollo.hip) against its siblings among the
element-wise kernels, over the 2-D matrices of a benchmark configuration (default C4) on the split
master, in the form of tools/adamini_ab.py.

ONE process, the same placed buffers (bf16 parameter, int16 residual, bf16 gradient), one kernel set
per variant over the same matrices, the variants interleaved in every round after one untimed
round, every launch between two HIP events.  Per variant: the median of each round, their median
and the spread (max - min) between rounds.

Variants: APOLLO at rank 256 per channel (``apollo_r256``) and at rank 1 per tensor
(``apollo_mini``), each of the four kernels of the rank-256 set alone (``a1_sketch``, ``a2_moments``,
``a3_finish``, ``a4_apply``), Adam-mini, Adam with bf16 moments and SGD with momentum over the same
matrices.  Nothing is gated.

Usage: python tools/apollo_ab.py [--rounds 5] [--steps 20] [--config C4] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))

PASSES = ("a1_sketch", "a2_moments", "a3_finish", "a4_apply")
VARIANTS = ("apollo_r256", "apollo_mini") + PASSES + ("adamini", "adam_bf16", "sgd_momentum")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--config", default="C4", choices=["C2", "C3", "C4", "C5"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"

    import numpy as np
    import torch

    from zero_amd import _lib
    from zero_amd.kernels import (AdamMiniSet, AdamSet, ApolloSet, SgdSet, adam_hparams,
                                  adamini_hparams, apollo_hparams, sgd_hparams)
    from zero_amd.shapes import CONFIGS

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    name, shape_fn = CONFIGS[args.config]
    shapes = [s for s in (tuple(int(x) for x in s) for s in shape_fn()) if len(s) == 2]
    numels = [s[0] * s[1] for s in shapes]
    offs, total = [], 0
    for n in numels:  # every matrix 256-byte aligned in every array
        offs.append(total)
        total += (n + 127) // 128 * 128
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    hi = torch.empty(total, dtype=torch.float32, device=dev).normal_(0.0, 0.02, generator=gen).to(
        torch.bfloat16)
    lo = torch.zeros(total, dtype=torch.int16, device=dev)
    g = (torch.empty(total, dtype=torch.float32, device=dev).normal_(generator=gen) * 1e-3).to(
        torch.bfloat16)
    m32 = torch.zeros(total, dtype=torch.float32, device=dev)
    mb = torch.zeros(total, dtype=torch.bfloat16, device=dev)
    vb = torch.zeros(total, dtype=torch.bfloat16, device=dev)
    BF16, SPLIT = _lib.ZS_BF16, _lib.ZS_BF16_SPLIT

    def apollo_set(rank: int):
        n = [(max(s) * rank + 3) // 4 * 4 for s in shapes]
        so = np.concatenate([[0], np.cumsum([2 * x + 4 for x in n])])
        state = torch.zeros(int(so[-1]), dtype=torch.float32, device=dev)
        rows = [[g.data_ptr() + 2 * o, hi.data_ptr() + 2 * o, lo.data_ptr() + 2 * o,
                 hi.data_ptr() + 2 * o, state.data_ptr() + 4 * int(b), state.data_ptr() + 4 * int(b + x),
                 state.data_ptr() + 4 * int(b + 2 * x), s[0], s[1], i, i]
                for i, (s, o, b, x) in enumerate(zip(shapes, offs, so, n))]
        return ApolloSet(np.array(rows, np.uint64), BF16, SPLIT, rank=rank), state

    def rows(m, v):
        r = np.zeros((len(numels), 9), np.uint64)
        o = np.asarray(offs, np.uint64)
        r[:, 0] = np.uint64(g.data_ptr()) + o * np.uint64(2)
        r[:, 1] = r[:, 3] = np.uint64(hi.data_ptr()) + o * np.uint64(2)
        r[:, 2] = np.uint64(lo.data_ptr()) + o * np.uint64(2)
        r[:, 4] = np.uint64(m.data_ptr()) + o * np.uint64(m.element_size())
        if v is not None:
            r[:, 5] = np.uint64(v.data_ptr()) + o * np.uint64(v.element_size())
        r[:, 8] = np.asarray(numels, np.uint64)
        return r

    a256, _s0 = apollo_set(256)
    a1, _s1 = apollo_set(1)
    voff = np.concatenate([[0], np.cumsum([(s[0] + 3) // 4 * 4 for s in shapes])])
    vblk = torch.zeros(int(voff[-1]), dtype=torch.float32, device=dev)
    mini = AdamMiniSet(np.array(
        [[g.data_ptr() + 2 * o, hi.data_ptr() + 2 * o, lo.data_ptr() + 2 * o, hi.data_ptr() + 2 * o,
          m32.data_ptr() + 4 * o, vblk.data_ptr() + 4 * int(vo), s[0], s[1], 1, i]
         for i, (s, o, vo) in enumerate(zip(shapes, offs, voff))], np.uint64), BF16, SPLIT)
    adam16 = AdamSet(rows(mb, vb), BF16, SPLIT, state_dtype=BF16)
    sgd = SgdSet(rows(m32, None), BF16, SPLIT)
    hp256, hp1 = apollo_hparams(1e-3), apollo_hparams(1e-3, scale=128.0, scale_type="tensor")
    mhp, shp = adamini_hparams(1e-3), sgd_hparams(1e-3, 0.9)
    st = torch.cuda.current_stream()
    count = {k: 0 for k in VARIANTS}
    elems = int(sum(numels))
    gbytes = 2 * elems  # one read of the bf16 gradient
    nbytes = {"apollo_r256": a256.bytes, "apollo_mini": a1.bytes,
              "a1_sketch": gbytes + 4 * a256.state_elems // 2,
              "a2_moments": 4 * a256.state_elems // 2 + 8 * a256.state_elems, "a3_finish": 0,
              "a4_apply": gbytes + 8 * elems, "adamini": mini.bytes, "adam_bf16": adam16.bytes,
              "sgd_momentum": sgd.bytes}

    def launch(k):
        count[k] += 1
        if k == "apollo_r256":
            a256.run(hp256, count[k], st)
        elif k == "apollo_mini":
            a1.run(hp1, count[k], st)
        elif k in PASSES:
            a256.run_pass(hp256, 7, PASSES.index(k), st)
        elif k == "adamini":
            mini.run(mhp, count[k], st)
        elif k == "sgd_momentum":
            sgd.run(shp, st)
        else:  # (beta2 0.99: within the bound of bf16 moments rounded to nearest)
            adam16.run(adam_hparams(1e-3, 0.9, 0.99, 1e-8, 0.0, count[k]), st)

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

    rounds = {k: [] for k in VARIANTS}
    for k in VARIANTS:  # one untimed round: code load, page tables, clocks
        block(k, args.steps)
    for r in range(args.rounds):
        for k in (VARIANTS if r % 2 == 0 else VARIANTS[::-1]):
            ms = block(k, args.steps)
            rounds[k].append(float(np.median(ms)))
            print(json.dumps({"round": r, "variant": k, "median_ms": rounds[k][-1], "min_ms": min(ms),
                              "max_ms": max(ms), "gbs": nbytes[k] / rounds[k][-1] / 1e6}), flush=True)
    summary = {"config": f"{args.config} {name}", "matrices": len(shapes), "params": elems,
               "master": "split", "rounds": args.rounds, "steps_per_round": args.steps,
               "sets": {k: {"rank": s.rank, "channels": s.channels, "scratch_bytes": s.scratch_bytes,
                            "sketch_workgroups": s.sketch_workgroups,
                            "state_bytes_per_param": 4 * s.state_elems / elems}
                        for k, s in (("apollo_r256", a256), ("apollo_mini", a1))},
               "sketch_flop": 2 * 256 * elems, "variants": {}}
    for k in VARIANTS:
        med = float(np.median(rounds[k]))
        summary["variants"][k] = {"round_medians_ms": rounds[k], "median_ms": med,
                                  "spread_ms": max(rounds[k]) - min(rounds[k]),
                                  "bytes_per_element": nbytes[k] / elems,
                                  "gbs": nbytes[k] / med / 1e6}
    summary["sketch_tflops"] = summary["sketch_flop"] / summary["variants"]["a1_sketch"]["median_ms"] / 1e9
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
