"""In-process A/B of the vector Adam kernel's diagnostic knobs on one C4-size ShardedOptimizer.

Placement differs from process to process (two runs of the same code can be ~3 % apart), so a
change of the kernel is judged here: ONE optimizer, so the same placed buffers, stepped in
alternating blocks with ``zs_tune("adam_loads_first")`` at 0 (every chunk through the predicated
body) and at 1 (full chunks through the loads-first body), optionally at several grids
(``zs_tune("adam_wg_per_cu")``).  Every launch is timed with HIP events around it (the engine's
``timing_events``).  One untimed round comes first (the first blocks after start-up run ~1 % slow
while clocks settle).  Per setting: the median of each round, their median, and the spread (max -
min) between rounds of that setting.  The gate for "setting B is faster than setting A": B's
median is below A's by more than three times the larger of the two spreads, and by at least 1 %.

Usage: python tools/adam_ab.py [--rounds 7] [--steps 30] [--settings 0:0,1:0,1:256,1:384]
                               [--config C4] [--master split] [--out FILE.json]
A setting is LOADS_FIRST:WG_PER_CU (0 = the kernel's default grid: 128 workgroups per CU for the
predicated kernel, 1024 for the loads-first one with a split master); the first one is the
baseline of the gate.
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--settings", default="0:0,1:0")
    ap.add_argument("--config", default="C4", choices=["C2", "C3", "C4", "C5"])
    ap.add_argument("--master", default="split", choices=["split", "fp32"])
    ap.add_argument("--port", type=int, default=29547)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"
    settings = [tuple(int(x) for x in s.split(":")) for s in args.settings.split(",")]

    import numpy as np
    import torch
    import torch.distributed as dist

    from zero_amd import _lib, zero2
    from zero_amd.shapes import CONFIGS

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{args.port}", rank=0, world_size=1)
    name, shape_fn = CONFIGS[args.config]
    shapes = shape_fn()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    params = [torch.nn.Parameter(torch.empty(s, dtype=torch.float32, device=dev).normal_(
        0.0, 0.02, generator=gen).to(torch.bfloat16)) for s in shapes]
    gen.manual_seed(1)
    grads = [(torch.empty(s, dtype=torch.float32, device=dev).normal_(generator=gen) * 1e-3).to(
        torch.bfloat16) for s in shapes]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), sync=False, master=args.master)
    if opt.engine is None:
        opt._build_engine()
    eng = opt.engine

    def step():
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()

    def tune(lf, wg):
        _lib.call("zs_tune", b"adam_loads_first", lf, None)
        _lib.call("zs_tune", b"adam_wg_per_cu", wg, None)

    def block(n):
        """n steps; the HIP-event time of each step's Adam launches, ms."""
        eng.timing_events = []
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        ev, eng.timing_events = eng.timing_events, None
        per = len(ev) // n
        ms = [e0.elapsed_time(e1) for e0, e1, _ in ev]
        return [sum(ms[i * per:(i + 1) * per]) for i in range(n)], sum(b for _, _, b in ev[:per])

    rounds = {s: [] for s in settings}
    nbytes = 0
    try:
        for s in settings:  # one untimed round: code load, page tables, clocks
            tune(*s)
            block(args.steps)
        for r in range(args.rounds):
            order = settings if r % 2 == 0 else settings[::-1]
            for s in order:
                tune(*s)
                ms, nbytes = block(args.steps)
                rounds[s].append(float(np.median(ms)))
                print(json.dumps({"round": r, "loads_first": s[0], "wg_per_cu": s[1] or "default",
                                  "median_ms": rounds[s][-1], "min_ms": min(ms), "max_ms": max(ms)}),
                      flush=True)
    finally:
        tune(1, 0)
    summary = {"config": f"{args.config} {name}", "params": int(sum(p.numel() for p in params)),
               "master": args.master, "adam_bytes_per_step": int(nbytes), "rounds": args.rounds,
               "steps_per_round": args.steps, "placement": getattr(eng, "placement", None),
               "settings": []}
    base = None
    for s in settings:
        med = float(np.median(rounds[s]))
        row = {"loads_first": s[0], "wg_per_cu": s[1] or "default", "round_medians_ms": rounds[s],
               "median_ms": med, "spread_ms": max(rounds[s]) - min(rounds[s]),
               "gbs": nbytes / med / 1e6}
        if base is None:
            base = row
        else:
            gain = base["median_ms"] - med
            noise = max(base["spread_ms"], row["spread_ms"])
            row["vs_first"] = {"gain_ms": gain, "gain_pct": 100.0 * gain / base["median_ms"],
                               "three_spreads_ms": 3.0 * noise,
                               "gate_met": bool(gain > 3.0 * noise and gain >= 0.01 * base["median_ms"])}
        summary["settings"].append(row)
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
