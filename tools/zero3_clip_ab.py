"""In-process A/B of gradient clipping and the guarded update in ZeRO-3 update mode: rank 0 of a
simulated ws-rank parameter set (default the C5 set at ws = 8) with the suite's simulated-rank
communicator (tests/_gloo_comm.py SimRankComm, as tools/accum_ab.py): a reduce-scatter is the copy
of this rank's chunk of every gradient and the norm's scalar all-reduce a no-op, so what is timed
is this rank's device work and the stream ordering around the all-reduce's place.

ONE optimizer, so the same placed buffers, stepped in alternating blocks with ``max_grad_norm`` at
None (the unclipped path), inf (the norm pass over this rank's chunks and the CLIP instances of
the update, coefficient 1) and inf with ``skip_nonfinite`` (the guarded coefficient kernel and the
GUARD instances).  Every iteration is one backward, a device synchronize, and ``step()`` between
two HIP events on the compute stream; the norm passes and the update launches are timed by events
of their own (``norm_events``, ``timing_events``).  One untimed round comes first.  Per setting:
the median of each round, their median and the spread between rounds; for the norm pass its median
time, bytes and rate.  The method is tools/clip_ab.py's.

Usage: python tools/zero3_clip_ab.py [--config C5] [--ws 8] [--rounds 7] [--steps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

SETTINGS = (("none", None, False), ("inf", float("inf"), False), ("inf+skip", float("inf"), True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C5")
    ap.add_argument("--ws", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 5, "at least 5 rounds of at least 5 steps"

    import numpy as np
    import torch
    import torch.distributed as dist

    import bench
    from _gloo_comm import SimRankComm
    from zero_amd import zero3 as z3
    from zero_amd.paramset import ParamSetModel, decoder_layer_groups
    from zero_amd.shapes import CONFIGS

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(bench._free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    dev = torch.device("cuda:0")
    shapes = CONFIGS[args.config][1]()
    ws = args.ws
    gen = torch.Generator(device=dev).manual_seed(0)
    params = [torch.nn.Parameter(torch.empty(s, device=dev, dtype=torch.bfloat16).normal_(
        0.0, 0.02, generator=gen)) for s in shapes]
    grads = [torch.empty(s, device=dev, dtype=torch.bfloat16).normal_(0.0, 1e-3, generator=gen)
             for s in shapes]
    model = ParamSetModel(params, decoder_layer_groups(len(shapes)))
    model.set_grad_source(grads)
    real_get = z3.get
    z3.get = lambda what, dm=None: {"ws": ws, "rank": 0}.get(what) if what in ("ws", "rank") \
        else real_get(what, dm)
    opt = z3.ShardedOptimizer(torch.optim.Adam(model.parameters(), lr=1e-3), update=True, sync=False,
                              comm=SimRankComm(ws, 0), max_grad_norm=float("inf"),
                              skip_nonfinite=True)
    z3.register_zero3_hooks(model, opt.param_managers)
    x = torch.zeros(1, device=dev, requires_grad=True)
    stream = torch.cuda.current_stream(dev)

    def block(setting, n):
        """n iterations under ``setting``: per step the ms of step(), of its norm passes and of
        its update launches; the norm's bytes."""
        _, limit, guard = setting
        opt.max_grad_norm = limit
        opt.skip_nonfinite = guard  # (the one optimizer serves both coefficient kernels)
        if opt._clip is not None:
            opt._clip.guard = guard
        step_ms, norm_ms, upd_ms, nbytes = [], [], [], 0
        for _ in range(n):
            model(x).sum().backward()
            torch.cuda.synchronize()
            opt.norm_events, opt.timing_events = [], []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            opt.step()
            e1.record(stream)
            torch.cuda.synchronize()
            step_ms.append(e0.elapsed_time(e1))
            norm_ms.append(sum(a.elapsed_time(b) for a, b, _ in opt.norm_events))
            upd_ms.append(sum(a.elapsed_time(b) for a, b, _ in opt.timing_events))
            nbytes = sum(b for _, _, b in opt.norm_events)
            assert nbytes == opt.last_norm_bytes
            opt.norm_events = opt.timing_events = None
            opt.zero_grad()
        return step_ms, norm_ms, upd_ms, nbytes

    keys = ("step", "norm", "update")
    rounds = {s[0]: {k: [] for k in keys} for s in SETTINGS}
    norm_bytes = {}
    block(SETTINGS[2], 1)  # (makes the clip stages with their counter: the guard can be switched)
    for s in SETTINGS:  # one untimed round: code load, page tables, clocks
        block(s, args.steps)
    for r in range(args.rounds):
        for s in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
            st, nm, up, nb = block(s, args.steps)
            for k, v in zip(keys, (st, nm, up)):
                rounds[s[0]][k].append(float(np.median(v)))
            norm_bytes[s[0]] = nb
            print(json.dumps({"round": r, "setting": s[0], "step_median_ms": rounds[s[0]]["step"][-1],
                              "norm_median_ms": rounds[s[0]]["norm"][-1],
                              "update_median_ms": rounds[s[0]]["update"][-1]}), flush=True)
    assert int(opt.skipped_steps.item()) == 0
    res = {"config": args.config, "simulated_ws": ws, "chunk_arena_elements": int(opt._arena.total),
           "update_bytes_per_step": int(opt._core.last_adam_bytes), "rounds": args.rounds,
           "steps_per_round": args.steps, "placement": getattr(opt, "placement", None),
           "settings": []}
    base = None
    for name, _, _ in SETTINGS:
        row = {"setting": name}
        for k in keys:
            v = rounds[name][k]
            row[k] = {"round_medians_ms": v, "median_ms": float(np.median(v)),
                      "spread_ms": max(v) - min(v)}
        nb = norm_bytes[name]
        if nb:
            row["norm"].update(bytes=int(nb), gbs=nb / row["norm"]["median_ms"] / 1e6)
        if base is None:
            base = row
        else:
            row["vs_none"] = {k + "_cost_ms": row[k]["median_ms"] - base[k]["median_ms"]
                              for k in ("step", "update")}
        res["settings"].append(row)
    print(json.dumps(res), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
