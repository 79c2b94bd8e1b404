"""In-process A/B of the stats instance of the fused Adam update (per-parameter update and weight
norms), at the kernel level.

ONE process and ONE set of buffers (placement differs from process to process by a few percent): a
flat shard of ``--elems`` elements (default: C4, SmolLM3-3B's 3,075,098,624 parameters, one segment
per parameter tensor) over the split master with bf16 gradients, over which alternating blocks time

    plain    zs_adamset_run                      26 B/element
    stats    zs_adamset_run_stats                26 B/element + two planes of 8-byte partials
    finish   the two zs_sqnorm_reduce_params launches and zs_update_norms (one parameter per segment)

The two update settings run over the same set.  Every launch (the three of ``finish`` together) is
timed with HIP events on the compute stream; a block is ``--steps`` launches, a round runs every
setting once, in alternating order; one untimed round comes first.  Per setting: the median of each
round, their median and the spread between rounds.  The yardstick of DESIGN.md §4: the plain instance
of the same run, the noise floor its own round-to-round spread.  Reported, not gated.

Usage: python tools/update_norms_ab.py [--rounds 7] [--steps 20] [--elems N] [--out FILE.json]
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
    ap.add_argument("--elems", type=int, default=0, help="0: the C4 parameter set")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5 and args.steps >= 10, "at least 5 rounds of at least 10 steps"

    import numpy as np
    import torch

    from zero_amd._lib import ZS_BF16, ZS_BF16_SPLIT
    from zero_amd._update import UpdateNorms
    from zero_amd.kernels import AdamSet, adam_hparams, sqnorm_reduce_params, update_norms
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
         "m": torch.zeros(N, device=dev), "v": torch.zeros(N, device=dev)}
    del w
    at = lambda name, k: T[name].data_ptr() + int(off[k]) * T[name].element_size()  # noqa: E731
    rows = np.array([[at("g", k), at("hi", k), at("lo", k), at("hi", k), at("m", k), at("v", k), 0, 0, n]
                     for k, n in enumerate(sizes)], dtype=np.uint64)
    aset = AdamSet(rows, ZS_BF16, ZS_BF16_SPLIT)
    so = aset.update_norm_offsets
    slots, npar = int(so[-1]), len(sizes)
    partials = torch.zeros(2 * slots, dtype=torch.float64, device=dev)
    csr, touched = UpdateNorms.tables([0], [so], [np.arange(npar)], npar)
    nr = (len(csr) - (npar + 1)) // 3
    csr = torch.from_numpy(csr).to(dev)
    sums3 = torch.zeros(3 * npar, device=dev)
    sums3[2 * npar:] = torch.from_numpy(touched).to(dev)
    un, wn = torch.zeros(npar, device=dev), torch.zeros(npar, device=dev)
    hp = adam_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 10)
    st = torch.cuda.current_stream(dev)

    def finish():
        for plane in (0, 1):
            sqnorm_reduce_params(partials, csr[:npar + 1],
                                 csr[npar + 1 + plane * nr:npar + 1 + (plane + 1) * nr],
                                 csr[npar + 1 + 2 * nr:], npar, sums3[plane * npar:], st)
        update_norms(sums3, npar, None, un, wn, st)

    run = {"plain": lambda: aset.run(hp, st),
           "stats": lambda: aset.run_stats(hp, partials, st),
           "finish": finish}
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
    summary = {"shard": label, "elems": elems, "segments": npar, "slots_per_plane": slots,
               "partials_bytes": 16 * slots, "rounds": args.rounds, "steps_per_round": args.steps,
               "settings": {}}
    for s in settings:
        med = float(np.median(rounds[s]))
        summary["settings"][s] = {"round_medians_ms": rounds[s], "median_ms": med,
                                  "spread_ms": max(rounds[s]) - min(rounds[s])}
        if s != "finish":
            summary["settings"][s].update(bytes_per_elem=26, gbs=26 * elems / med / 1e6)
    S = summary["settings"]
    diff = S["stats"]["median_ms"] - S["plain"]["median_ms"]
    summary["stats_vs_plain"] = {"diff_ms": diff, "plain_spread_ms": S["plain"]["spread_ms"],
                                 "within_plain_spread": abs(diff) <= S["plain"]["spread_ms"],
                                 "ratio": S["stats"]["median_ms"] / S["plain"]["median_ms"]}
    summary["per_step_cost_ms"] = diff + S["finish"]["median_ms"]
    norms = torch.stack([un, wn]).cpu().numpy()
    summary["sane"] = bool(np.isfinite(norms).all() and (norms[1] > 0).all())
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
