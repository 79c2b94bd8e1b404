"""GPU cost of an accumulating pass of ZeRO-3 update mode (``grad_accumulation=True``) beside the
first pass, in one run: rank 0 of a simulated ws-rank parameter set (default the C5 set at ws = 8),
with the suite's simulated-rank communicator (tests/_gloo_comm.py SimRankComm, as
tests/test_gpu_zero3.py's C5 case): a reduce-scatter is the copy of this rank's chunk of every
gradient (every other rank contributes zeros), so the reduce side of a pass is real device work on
the reducing stream.

Every step runs a first pass (chunks land in the grad chunk arena) and an accumulating pass (chunks
land in the staging buffer, then one zs_accumulate per bucket over the bucket's range of the arena).
Per bucket, HIP events on the reducing stream bracket the collective and, for the accumulating
pass, the add (the reducer's ``timing`` hook); the tool sums them per pass and reports, per step and
as medians, the first pass's reduce side, the accumulating pass's, and their difference — the
price of the extra pass over the chunk arena.  The two passes alternate within every step, so the
box's drift affects both alike.

Prediction written before any run: about 1.0e9 bf16 chunk elements x 6 B at about 6 TB/s, roughly
1 ms per accumulating pass of the C5 set at ws = 8.

``--fp32``: the optimizer is built with ``accumulation_dtype=torch.float32`` and every step takes
three passes; steps alternate between fp32 accumulation (zs_accumulate_widen: the second pass reads
the bf16 arena and the staging buffer, 8 B per element, the third the fp32 arena and the staging
buffer, 10 B) and bf16 accumulation (zs_accumulate, 6 B, the reducer's ``widen`` switched off for
that step), so both run in one process on the same buffers.  The update of every step is timed as
well (``timing_events``): the fp32-gradient split-master instance after an fp32 step, the
bf16-gradient one after a bf16 step.  Predictions written before any run, from the bf16 pass's
measured 0.86 ms for 1.004e9 elements at 6 B: about 1.15 ms for the 8-B pass, about 1.4 ms for the
10-B pass, and 28 / 26 = 1.08 x for the update.

Usage: python tools/accum_ab.py [--config C5] [--ws 8] [--steps 8] [--warmup 2] [--fp32] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C5")
    ap.add_argument("--ws", type=int, default=8)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fp32", action="store_true",
                    help="alternate fp32 and bf16 accumulation, three passes per step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

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
                              comm=SimRankComm(ws, 0), grad_accumulation=True,
                              accumulation_dtype=torch.float32 if args.fp32 else None)
    z3.register_zero3_hooks(model, opt.param_managers)
    red = opt._reducer
    x = torch.zeros(1, device=dev, requires_grad=True)
    chunk_elems = int(opt._arena.total)
    rows = []
    if args.fp32:
        res = fp32_ab(args, torch, opt, model, x, chunk_elems)
        print(json.dumps({k: v for k, v in res.items() if k != "steps"}), flush=True)
        if args.out:
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
        dist.destroy_process_group()
        return
    for step in range(args.warmup + args.steps):
        per_pass = []
        for _ in range(2):
            red.timing = []
            model(x).sum().backward()
            torch.cuda.synchronize()
            per_pass.append(sum(e0.elapsed_time(e1) for e0, e1, _ in red.timing))
            assert len(red.timing) == red.K
        red.timing = None
        assert opt.accumulated_passes == 2
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        if step >= args.warmup:
            rows.append({"step": step - args.warmup, "first_pass_reduce_ms": round(per_pass[0], 4),
                         "accumulating_pass_reduce_ms": round(per_pass[1], 4),
                         "extra_ms": round(per_pass[1] - per_pass[0], 4)})
            print(json.dumps(rows[-1]), flush=True)

    def med(key):
        v = sorted(r[key] for r in rows)
        return v[len(v) // 2]

    es = opt.grad_arena().element_size()
    extra = med("extra_ms")
    res = {"config": args.config, "simulated_ws": ws, "buckets": red.K,
           "chunk_arena_elements": chunk_elems, "staging_elements": int(opt.grad_staging().numel()),
           "accumulate_launches_per_pass": red.K,
           "first_pass_reduce_ms_median": med("first_pass_reduce_ms"),
           "accumulating_pass_reduce_ms_median": med("accumulating_pass_reduce_ms"),
           "extra_ms_median": extra,
           "extra_gbs_over_3x_chunk_bytes": round(3 * chunk_elems * es / (extra / 1e3) / 1e9, 1)
           if extra > 0 else None,
           "predicted_extra_ms": round(chunk_elems * 3 * es / 6e12 * 1e3, 3)}
    print(json.dumps(res), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(dict(res, steps=rows), indent=1) + "\n")
    dist.destroy_process_group()


def fp32_ab(args, torch, opt, model, x, chunk_elems):
    """Three passes per step, steps alternating fp32 / bf16 accumulation; per step the reduce side
    of each pass and the update's launches."""
    red = opt._reducer
    assert red.widen, "the set has no bf16 chunk arena at ws > 1"
    rows = []
    for step in range(2 * (args.warmup + args.steps)):
        wide = step % 2 == 0
        red.widen = opt._acc_widen = wide  # (the fp32 arena stays allocated either way)
        per_pass = []
        for _ in range(3):
            red.timing = []
            model(x).sum().backward()
            torch.cuda.synchronize()
            per_pass.append(sum(e0.elapsed_time(e1) for e0, e1, _ in red.timing))
        red.timing = None
        assert opt.grad_arena().dtype == (torch.float32 if wide else torch.bfloat16)
        opt.timing_events = []
        opt.step()
        torch.cuda.synchronize()
        upd = sum(e0.elapsed_time(e1) for e0, e1, _ in opt.timing_events)
        upd_bytes = sum(b for _, _, b in opt.timing_events)
        opt.timing_events = None
        opt.zero_grad()
        if step >= 2 * args.warmup:
            rows.append({"step": step - 2 * args.warmup, "accumulation": "fp32" if wide else "bf16",
                         "first_pass_reduce_ms": round(per_pass[0], 4),
                         "second_pass_extra_ms": round(per_pass[1] - per_pass[0], 4),
                         "third_pass_extra_ms": round(per_pass[2] - per_pass[0], 4),
                         "update_ms": round(upd, 4), "update_bytes": int(upd_bytes)})
            print(json.dumps(rows[-1]), flush=True)
    red.widen = opt._acc_widen = True

    def med(kind, key):
        v = sorted(r[key] for r in rows if r["accumulation"] == kind)
        return v[len(v) // 2]

    res = {"config": args.config, "simulated_ws": args.ws, "buckets": red.K,
           "chunk_arena_elements": chunk_elems,
           "predicted_ms": {"bf16_pass_6B": 0.86, "fp32_second_pass_8B": 1.15,
                            "fp32_third_pass_10B": 1.4, "update_ratio": 1.08}}
    for kind, b2, b3 in (("bf16", 6, 6), ("fp32", 8, 10)):
        e2, e3, u = med(kind, "second_pass_extra_ms"), med(kind, "third_pass_extra_ms"), med(kind, "update_ms")
        ub = med(kind, "update_bytes")
        res[kind] = {"second_pass_extra_ms_median": e2, "third_pass_extra_ms_median": e3,
                     "second_pass_gbs": round(b2 * chunk_elems / (e2 / 1e3) / 1e9, 1) if e2 > 0 else None,
                     "third_pass_gbs": round(b3 * chunk_elems / (e3 / 1e3) / 1e9, 1) if e3 > 0 else None,
                     "update_ms_median": u, "update_bytes": ub,
                     "update_gbs": round(ub / (u / 1e3) / 1e9, 1) if u > 0 else None}
    res["update_ratio_fp32_over_bf16"] = round(res["fp32"]["update_ms_median"]
                                               / res["bf16"]["update_ms_median"], 4)
    res["steps"] = rows
    return res


if __name__ == "__main__":
    main()
