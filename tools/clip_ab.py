"""In-process A/B of global gradient-norm clipping on one C4-size ShardedOptimizer.

ONE optimizer, so the same placed buffers (placement differs from process to process by ~3 %),
stepped in alternating blocks with ``max_grad_norm`` at None (the unclipped path), inf (the norm
pass and the CLIP instance of the update, coefficient 1) and 1.0 (the same with a coefficient well
below 1).  Every step is timed with HIP events around ``step()`` on the compute stream, every norm
pass with events around its launch (the engine's ``norm_events``).  One untimed round comes first.
Per setting: the median of each round, their median and the spread between rounds; for the norm
pass its median time, bytes and rate against the 8 TB/s peak.

Usage: python tools/clip_ab.py [--rounds 7] [--steps 30] [--settings none,inf,1.0,inf:0]
                               [--config C4] [--master split] [--out FILE.json]
A setting is LIMIT[:NT]; NT is ``zs_tune("sqnorm_nt")``, the cache policy of the pass's loads
(1, the default: non-temporal; 0: the default policy).  The first setting is the baseline.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))


def _lim(x):
    """``max_grad_norm`` as JSON: None, a number, or "inf"."""
    return "inf" if x is not None and x == float("inf") else x


def parse_setting(s: str):
    limit, _, nt = s.partition(":")
    return (None if limit.lower() == "none" else float(limit)), (int(nt) if nt else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--settings", default="none,inf,1.0")
    ap.add_argument("--config", default="C4", choices=["C2", "C3", "C4", "C5"])
    ap.add_argument("--master", default="split", choices=["split", "fp32"])
    ap.add_argument("--port", type=int, default=29548)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"
    settings = [parse_setting(s) for s in args.settings.split(",")]

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
    stream = torch.cuda.current_stream(dev)

    def block(setting, n):
        """n steps under ``setting``: ms per step, ms per step in the norm passes, norm bytes."""
        limit, nt = setting
        opt.max_grad_norm = limit
        _lib.call("zs_tune", b"sqnorm_nt", nt, None)
        eng.norm_events = []
        ev = []
        for _ in range(n):
            for p, g in zip(params, grads):
                p.grad = g
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            opt.step()
            e1.record(stream)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        nev, eng.norm_events = eng.norm_events, None
        per = len(nev) // n
        nms = [a.elapsed_time(b) for a, b, _ in nev]
        norm_ms = [sum(nms[i * per:(i + 1) * per]) for i in range(n)] if per else []
        return [a.elapsed_time(b) for a, b in ev], norm_ms, sum(b for _, _, b in nev[:per])

    rounds = {s: [] for s in settings}
    norm_rounds = {s: [] for s in settings}
    norm_bytes = {s: 0 for s in settings}
    seen = {}
    try:
        for s in settings:  # one untimed round: code load, page tables, clocks
            block(s, args.steps)
        for r in range(args.rounds):
            order = settings if r % 2 == 0 else settings[::-1]
            for s in order:
                ms, nms, nb = block(s, args.steps)
                rounds[s].append(float(np.median(ms)))
                if nms:
                    norm_rounds[s].append(float(np.median(nms)))
                    norm_bytes[s] = nb
                    seen[s] = (float(opt.last_grad_norm.item()), float(opt.last_clip_coef.item()))
                print(json.dumps({"round": r, "max_grad_norm": _lim(s[0]), "sqnorm_nt": s[1],
                                  "median_ms": rounds[s][-1], "min_ms": min(ms), "max_ms": max(ms),
                                  "norm_median_ms": norm_rounds[s][-1] if nms else None}),
                      flush=True)
    finally:
        _lib.call("zs_tune", b"sqnorm_nt", 1, None)
    summary = {"config": f"{args.config} {name}", "params": int(sum(p.numel() for p in params)),
               "master": args.master, "adam_bytes_per_step": int(eng.last_adam_bytes),
               "rounds": args.rounds, "steps_per_round": args.steps,
               "placement": getattr(eng, "placement", None), "settings": []}
    base = None
    for s in settings:
        med = float(np.median(rounds[s]))
        row = {"max_grad_norm": _lim(s[0]), "sqnorm_nt": s[1], "round_medians_ms": rounds[s],
               "median_ms": med, "spread_ms": max(rounds[s]) - min(rounds[s])}
        if norm_rounds[s]:
            nmed = float(np.median(norm_rounds[s]))
            row["norm_pass"] = {"round_medians_ms": norm_rounds[s], "median_ms": nmed,
                                "spread_ms": max(norm_rounds[s]) - min(norm_rounds[s]),
                                "bytes": int(norm_bytes[s]), "gbs": norm_bytes[s] / nmed / 1e6,
                                "frac_of_8tbs": norm_bytes[s] / nmed / 1e6 / 8000.0}
            row["last_grad_norm"], row["last_clip_coef"] = seen[s]
        if base is None:
            base = row
        else:
            row["vs_first"] = {"cost_ms": med - base["median_ms"],
                               "cost_pct": 100.0 * (med - base["median_ms"]) / base["median_ms"]}
        summary["settings"].append(row)
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
