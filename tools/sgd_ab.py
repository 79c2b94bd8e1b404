"""In-process A/B of the fused SGD and the fused Adam update on one C4-size parameter set.

ONE ZeRO-2 optimizer at world size 1 is built, so parameters, residuals and state are placed once
(placement differs from process to process by ~3 %).  Over its arena three kernel sets are made
from the engine's own rows: the Adam set (exp_avg, exp_avg_sq), an SGD set whose momentum buffer is
the exp_avg array, and an SGD set without buffers.  They run in alternating blocks on the same
buffers and the same gradients, every launch timed with HIP events on the compute stream.  One
untimed round comes first.  Per setting: the median of each round, their median, the spread
between rounds, the algorithmic bytes (zs_adamset_stats) and the rate against the 8 TB/s peak.

Usage: python tools/sgd_ab.py [--rounds 7] [--steps 30] [--settings adam,sgd,sgd0]
                              [--config C4] [--master split] [--out FILE.json]
A setting is KIND[:WG[:LF]]: KIND adam, sgd (momentum 0.9) or sgd0 (no momentum, no buffer); WG is
``zs_tune("adam_wg_per_cu")`` (0, the default: the kernels' own grid) and LF
``zs_tune("adam_loads_first")`` (1, the default).  The first setting is the baseline.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))

PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--settings", default="adam,sgd,sgd0")
    ap.add_argument("--config", default="C4", choices=["C2", "C3", "C4", "C5"])
    ap.add_argument("--master", default="split", choices=["split", "fp32"])
    ap.add_argument("--port", type=int, default=29549)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"
    settings = args.settings.split(",")
    assert len(set(settings)) == len(settings)

    def parse(s):
        kind, _, rest = s.partition(":")
        wg, _, lf = rest.partition(":")
        assert kind in ("adam", "sgd", "sgd0"), s
        return kind, int(wg) if wg else 0, int(lf) if lf else 1
    parsed = {s: parse(s) for s in settings}

    import numpy as np
    import torch
    import torch.distributed as dist

    from zero_amd import _lib, zero2
    from zero_amd.kernels import AdamSet, SgdSet, adam_hparams, sgd_hparams
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
    assert eng.ws == 1 and eng.K == 1
    stream = torch.cuda.current_stream(dev)
    rd = eng.rounds[0]
    rows = rd.rows.copy()  # the engine's rows over its placed arena; gradients read in place
    rows[:, 0] = np.fromiter((grads[int(i)].data_ptr() for i in rd.idx), np.uint64, len(rd.idx))
    sgd_rows = rows.copy()
    sgd_rows[:, 5] = 0  # no exp_avg_sq; column m (exp_avg) is the momentum buffer
    sgd0_rows = sgd_rows.copy()
    sgd0_rows[:, 4] = 0
    sets = {"adam": AdamSet(rows, eng.zdtype, eng.p_dtype),
            "sgd": SgdSet(sgd_rows, eng.zdtype, eng.p_dtype),
            "sgd0": SgdSet(sgd0_rows, eng.zdtype, eng.p_dtype)}
    count = {s: 0 for s in settings}

    def hp(s):
        count[s] += 1
        kind = parsed[s][0]
        if kind == "adam":
            return adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, count[s])
        return sgd_hparams(1e-4, 0.9 if kind == "sgd" else 0.0, first=count[s] == 1)

    def block(s, n):
        kind, wg, lf = parsed[s]
        _lib.call("zs_tune", b"adam_wg_per_cu", wg, None)
        _lib.call("zs_tune", b"adam_loads_first", lf, None)
        ev = []
        try:
            for _ in range(n):
                h = hp(s)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                sets[kind].run(h, stream)
                e1.record(stream)
                ev.append((e0, e1))
            torch.cuda.synchronize()
        finally:
            _lib.call("zs_tune", b"adam_wg_per_cu", 0, None)
            _lib.call("zs_tune", b"adam_loads_first", 1, None)
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
    n_el = int(sum(p.numel() for p in params))
    summary = {"config": f"{args.config} {name}", "params": n_el, "master": args.master,
               "rounds": args.rounds, "steps_per_round": args.steps,
               "placement": getattr(eng, "placement", None), "settings": []}
    base = None
    for s in settings:
        med = float(np.median(rounds[s]))
        nbytes = sets[parsed[s][0]].bytes
        gbs = nbytes / med / 1e6
        row = {"setting": s, "wg_per_cu": parsed[s][1], "loads_first": parsed[s][2],
               "round_medians_ms": rounds[s], "median_ms": med,
               "spread_ms": max(rounds[s]) - min(rounds[s]), "bytes": int(nbytes),
               "bytes_per_element": nbytes / n_el, "gbs": gbs,
               "frac_of_8tbs": gbs / PEAK_GBS,
               "frac_round_min_max": [nbytes / m / 1e6 / PEAK_GBS
                                      for m in (max(rounds[s]), min(rounds[s]))]}
        if base is None:
            base = row
        else:
            row["vs_first"] = {"ms": med - base["median_ms"],
                               "frac_of_8tbs": row["frac_of_8tbs"] - base["frac_of_8tbs"]}
        summary["settings"].append(row)
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
