"""In-process A/B of the gradient-norm pass with and without per-parameter norms on one C4-size
ShardedOptimizer.

ONE optimizer, so the same placed buffers and the same kernel sets (placement differs from
process to process by ~3 %): the sets of one clipped step are collected once, then the unsegmented
pass (zs_adamset_grad_sqnorm, ``max_grad_norm`` alone) and the segmented pass
(zs_adamset_grad_sqnorm_segs, ``param_grad_norms=True``) run over them in alternating blocks, each
pass between two HIP events; the reducers — zs_sqnorm_reduce alone against
zs_sqnorm_reduce_params + zs_sqnorm_reduce + zs_param_norms — are timed the same way.  One
untimed round comes first.  Per variant: the median of each round, their median and the spread
between rounds.  The yardstick of the segmented pass is the unsegmented one of the same run.

Usage: python tools/param_norms_ab.py [--rounds 7] [--steps 20] [--config C4] [--master split]
                                      [--out FILE.json]
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--config", default="C4", choices=["C2", "C3", "C4", "C5"])
    ap.add_argument("--master", default="split", choices=["split", "fp32"])
    ap.add_argument("--port", type=int, default=29549)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"

    import numpy as np
    import torch
    import torch.distributed as dist

    from zero_amd import zero2
    from zero_amd._update import GradClip
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
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3), sync=False, master=args.master,
                                 max_grad_norm=float("inf"))
    for p, g in zip(params, grads):
        p.grad = g
    opt.step()  # builds the engine and its sets, binds the gradients
    torch.cuda.synchronize()
    eng = opt.engine
    stream = torch.cuda.current_stream(dev)
    # the sets of a clipped step, as the engine collects them
    sets = [aset for rd in eng.rounds for _, _, aset in eng._static_sets(rd)]
    deferred = [(aset, None, None) for aset in sets]
    clips = {"unsegmented": GradClip(eng), "segmented": GradClip(eng, per_param=True)}
    clips["unsegmented"].prepare(deferred)
    clips["segmented"].prepare(deferred, [aset.seg_params for aset in sets])
    nbytes = sum(aset.grad_bytes for aset in sets)

    def block(which, n):
        """n norm passes and n reductions of variant ``which``: (ms per pass, ms per reduction)."""
        clip = clips[which]
        ev = []
        for _ in range(n):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(stream)
            clip.norm(deferred, 0, stream)
            e[1].record(stream)
            e[2].record(stream)
            clip.reduce(stream)
            clip.coef(float("inf"), stream)
            e[3].record(stream)
            ev.append(e)
        torch.cuda.synchronize()
        return [e[0].elapsed_time(e[1]) for e in ev], [e[2].elapsed_time(e[3]) for e in ev]

    order = list(clips)
    rounds = {w: {"pass": [], "reduce": []} for w in order}
    for w in order:  # one untimed round: code load, page tables, clocks
        block(w, args.steps)
    for r in range(args.rounds):
        for w in (order if r % 2 == 0 else order[::-1]):
            ms, rms = block(w, args.steps)
            rounds[w]["pass"].append(float(np.median(ms)))
            rounds[w]["reduce"].append(float(np.median(rms)))
            print(json.dumps({"round": r, "variant": w, "pass_median_ms": rounds[w]["pass"][-1],
                              "pass_min_ms": min(ms), "pass_max_ms": max(ms),
                              "reduce_median_ms": rounds[w]["reduce"][-1]}), flush=True)
    seg = clips["segmented"]
    summary = {"config": f"{args.config} {name}", "params": int(sum(p.numel() for p in params)),
               "tensors": len(params), "sets": len(sets), "master": args.master,
               "rounds": args.rounds, "steps_per_round": args.steps, "grad_bytes": int(nbytes),
               "partials": {w: int(clips[w]._off[-1]) for w in order},
               "global_norm": {w: float(clips[w].out[0].item()) for w in order},
               "param_norms_min_max": [float(seg.param_norms.min().item()),
                                       float(seg.param_norms.max().item())],
               "placement": getattr(eng, "placement", None), "variants": {}}
    for w in order:
        row = {}
        for what in ("pass", "reduce"):
            v = rounds[w][what]
            row[what] = {"round_medians_ms": v, "median_ms": float(np.median(v)),
                         "spread_ms": max(v) - min(v)}
        row["pass"]["gbs"] = nbytes / row["pass"]["median_ms"] / 1e6
        row["pass"]["frac_of_8tbs"] = row["pass"]["gbs"] / 8000.0
        summary["variants"][w] = row
    a, b = summary["variants"]["unsegmented"]["pass"], summary["variants"]["segmented"]["pass"]
    summary["segmented_vs_unsegmented"] = {
        "pass_cost_ms": b["median_ms"] - a["median_ms"],
        "pass_cost_pct": 100.0 * (b["median_ms"] - a["median_ms"]) / a["median_ms"],
        "unsegmented_spread_ms": a["spread_ms"],
        "within_spread": b["median_ms"] - a["median_ms"] <= a["spread_ms"],
        "reduce_cost_ms": summary["variants"]["segmented"]["reduce"]["median_ms"]
        - summary["variants"]["unsegmented"]["reduce"]["median_ms"]}
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
