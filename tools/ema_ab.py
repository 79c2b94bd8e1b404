"""In-process A/B of the EMA instance of the fused Adam update, at the kernel level.

ONE process and ONE set of buffers (placement differs from process to process by a few percent): a
flat shard of ``--elems`` elements (default: C4, SmolLM3-3B's 3,075,098,624 parameters, one segment
per parameter tensor), over which alternating blocks time

  split master (bf16 gradients):
    plain    zs_adamset_run                      26 B/element
    amsgrad  zs_adamset_run, hp.amsgrad          34 B/element  (vmax = the array the EMA uses)
    ema      zs_adamset_run_ema                  34 B/element
  fp32 master + bf16 parameter out (``--fp32-master``, on by default):
    plain32  zs_adamset_run                      28 B/element
    unfused  plain32 + torch ``ema.lerp_(master, w)``   28 + 12 B/element, two launches
    ema32    zs_adamset_run_ema                  36 B/element

Every launch (pair) is timed with HIP events on the compute stream; a block is ``--steps`` launches,
a round runs every setting once, in alternating order; one untimed round comes first.  Per setting:
the median of each round, their median and the spread between rounds.  The bar of DESIGN.md §4: the
EMA instance against the amsgrad instance of the same run, the margin the amsgrad instance's own
round-to-round spread; the fused-versus-unfused ratio is reported only.

Usage: python tools/ema_ab.py [--rounds 7] [--steps 20] [--elems N] [--decay 0.999]
                              [--no-fp32-master] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))

BYTES = {"plain": 26, "amsgrad": 34, "ema": 34, "plain32": 28, "unfused": 40, "ema32": 36}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--elems", type=int, default=0, help="0: the C4 parameter set")
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--no-fp32-master", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 10, "at least 5 rounds of at least 10 steps"

    import numpy as np
    import torch

    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT
    from zero_amd._update import ema_weight
    from zero_amd.kernels import AdamSet, adam_hparams
    from zero_amd.shapes import CONFIGS

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if args.elems:
        sizes, label = [int(args.elems)], f"{args.elems} elements, one segment"
    else:
        sizes = [int(np.prod(s)) for s in CONFIGS["C4"][1]()]
        label = "C4 " + CONFIGS["C4"][0]
    off = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 for n in sizes])]).astype(np.int64)
    N = int(off[-1])
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    w = torch.empty(N, dtype=torch.float32, device=dev).normal_(0.0, 0.02, generator=gen)
    T = {"hi": w.to(torch.bfloat16), "lo": torch.zeros(N, dtype=torch.int16, device=dev),
         "g": (torch.empty(N, dtype=torch.float32, device=dev).normal_(generator=gen) * 1e-3).to(
             torch.bfloat16),
         "m": torch.zeros(N, device=dev), "v": torch.zeros(N, device=dev), "x": w.clone()}
    fp32 = not args.no_fp32_master
    if fp32:
        T["master"], T["x2"] = w.clone(), w.clone()
    del w
    at = lambda name, k: T[name].data_ptr() + int(off[k]) * T[name].element_size()  # noqa: E731

    def rows(split, x):
        out = []
        for k, n in enumerate(sizes):
            head = [at("g", k), at("hi", k), at("lo", k), at("hi", k)] if split else \
                [at("g", k), at("master", k), at("master", k), at("hi", k)]
            out.append(head + [at("m", k), at("v", k), at(x, k) if x else 0, 0, n])
        return np.array(out, dtype=np.uint64)

    sets = {"plain": AdamSet(rows(True, None), ZS_BF16, ZS_BF16_SPLIT),
            "x": AdamSet(rows(True, "x"), ZS_BF16, ZS_BF16_SPLIT)}
    if fp32:
        sets["plain32"] = AdamSet(rows(False, None), ZS_BF16, ZS_BF16)
        sets["x32"] = AdamSet(rows(False, "x"), ZS_BF16, ZS_BF16)
    hp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 10)
    hp_ams = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 10, amsgrad=True)
    wgt = ema_weight(args.decay)
    st = torch.cuda.current_stream(dev)

    def unfused():
        sets["plain32"].run(hp, st)
        T["x2"].lerp_(T["master"], wgt)

    run = {"plain": lambda: sets["plain"].run(hp, st),
           "amsgrad": lambda: sets["x"].run(hp_ams, st),
           "ema": lambda: sets["x"].run_ema(hp, wgt, st)}
    if fp32:
        run.update(plain32=lambda: sets["plain32"].run(hp, st), unfused=unfused,
                   ema32=lambda: sets["x32"].run_ema(hp, wgt, st))
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
    summary = {"shard": label, "elems": elems, "segments": len(sizes), "decay": args.decay,
               "rounds": args.rounds, "steps_per_round": args.steps, "settings": {}}
    for s in settings:
        med = float(np.median(rounds[s]))
        summary["settings"][s] = {
            "bytes_per_elem": BYTES[s], "round_medians_ms": rounds[s], "median_ms": med,
            "spread_ms": max(rounds[s]) - min(rounds[s]),
            "gbs": BYTES[s] * elems / med / 1e6, "frac_of_8tbs": BYTES[s] * elems / med / 1e6 / 8000.0}
    S = summary["settings"]
    summary["ema_vs_amsgrad"] = {
        "diff_ms": S["ema"]["median_ms"] - S["amsgrad"]["median_ms"],
        "amsgrad_spread_ms": S["amsgrad"]["spread_ms"],
        "within_amsgrad_spread": abs(S["ema"]["median_ms"] - S["amsgrad"]["median_ms"])
        <= S["amsgrad"]["spread_ms"]}
    summary["ema_vs_plain_ms"] = S["ema"]["median_ms"] - S["plain"]["median_ms"]
    if fp32:
        summary["fused_over_unfused"] = S["ema32"]["median_ms"] / S["unfused"]["median_ms"]
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
