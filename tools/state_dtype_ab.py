"""In-process A/B of the fused Adam with fp32 and with bf16 moments on one C4-size parameter set.

ONE ZeRO-2 optimizer at world size 1 is built, so parameters, residuals and state are placed once
(placement differs from process to process by ~3 %).  Over its arena three kernel sets are made
from the engine's own rows: the fp32-state set, a second fp32-state set over the same rows (the
A/B's own spread: what two equal settings differ by), and a bf16-state set whose ``m`` and ``v`` lie
over the front halves of the same exp_avg / exp_avg_sq arrays.  They run in alternating blocks on
the same buffers and the same gradients, every launch timed with HIP events on the compute stream.
One untimed round comes first.  Per setting: the median of each round, their median, the spread
between rounds, the algorithmic bytes (zs_adamset_stats) and the rate against the 8 TB/s peak; then
the verdict: is bf16 state faster than fp32 state in every round by more than the largest
fp32-against-fp32 difference of any round?

``--sr`` (stochastic rounding of the bf16 moments): the settings are the fp32-state set, a bf16-state
set rounded to nearest, a second one over the same rows (the A/B's own spread) and a bf16-state set
run through zs_adamset_run_sr with torch's default betas; the verdict: is the stochastic step faster
than the fp32-state step in every round, and what is its ratio to the nearest one beside the spread
of the two equal nearest sets?

``--psr`` (master-free bf16 parameters, ``master="none"``; --kind split): the split-master sets with
bf16-stochastic moments (18 B/element, twice: the A/B's own spread) and with fp32 moments (26)
against master-free sets over the same rows — the same parameter arena and moment arrays, no
residual — with bf16-stochastic moments (14) and with fp32 moments (22), interleaved; the verdict:
is each master-free step faster than its split twin in every round by more than the spread of the
two equal split sets, and what are the time and byte ratios?

Usage: python tools/state_dtype_ab.py [--rounds 7] [--steps 30] [--kind split|fp32]
                                      [--config C4] [--sr | --psr] [--out FILE.json]
``--kind split``: bf16 parameters with the split master, bf16 gradients (26 against 18 B/element);
``--kind fp32``: fp32 parameters and gradients (28 against 20).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))

PEAK_GBS = 8000.0
SETTINGS = ("f32", "f32_again", "bf16")
SR_SETTINGS = ("f32", "bf16", "bf16_again", "bf16_sr")
PSR_SETTINGS = ("split_sr", "none_sr", "split_sr_again", "split_f32", "none_f32")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--kind", default="split", choices=["split", "fp32"])
    ap.add_argument("--config", default="C4", choices=["C2", "C3", "C4", "C5"])
    ap.add_argument("--port", type=int, default=29551)
    ap.add_argument("--sr", action="store_true")
    ap.add_argument("--psr", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    SETTINGS = SR_SETTINGS if args.sr else PSR_SETTINGS if args.psr else globals()["SETTINGS"]
    assert not (args.sr and args.psr) and (not args.psr or args.kind == "split")
    assert args.rounds >= 5 and args.steps >= 20, "at least 5 rounds of at least 20 steps"

    import numpy as np
    import torch
    import torch.distributed as dist

    from zero_amd import _lib, zero2
    from zero_amd.kernels import AdamSet, adam_hparams, sr_keys
    from zero_amd.shapes import CONFIGS

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{args.port}", rank=0, world_size=1)
    name, shape_fn = CONFIGS[args.config]
    shapes = shape_fn()
    pdt = torch.bfloat16 if args.kind == "split" else torch.float32
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    params = [torch.nn.Parameter(torch.empty(s, dtype=torch.float32, device=dev).normal_(
        0.0, 0.02, generator=gen).to(pdt)) for s in shapes]
    gen.manual_seed(1)
    grads = [(torch.empty(s, dtype=torch.float32, device=dev).normal_(generator=gen) * 1e-3).to(pdt)
             for s in shapes]
    opt = zero2.ShardedOptimizer(torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.95)), sync=False)
    if opt.engine is None:
        opt._build_engine()
    eng = opt.engine
    assert eng.ws == 1 and eng.K == 1 and eng.split == (args.kind == "split")
    stream = torch.cuda.current_stream(dev)
    rd = eng.rounds[0]
    rows = rd.rows.copy()  # the engine's rows over its placed arena; gradients read in place
    rows[:, 0] = np.fromiter((grads[int(i)].data_ptr() for i in rd.idx), np.uint64, len(rd.idx))
    half = rows.copy()  # bf16 m and v: the same shard offsets, 2 bytes an element
    for col, t in ((4, eng.m), (5, eng.v)):
        base = np.uint64(t.data_ptr())
        half[:, col] = base + (rows[:, col] - base) // np.uint64(2)
    mk16 = lambda: AdamSet(half, eng.zdtype, eng.p_dtype, state_dtype=_lib.ZS_BF16)  # noqa: E731
    sets = {"f32": AdamSet(rows, eng.zdtype, eng.p_dtype)}
    if args.psr:
        def free(r, **kw):  # the same rows without a master: the bf16 parameter in and out
            r = r.copy()
            r[:, 2] = 0
            assert np.array_equal(r[:, 1], r[:, 3])
            return AdamSet(r, eng.zdtype, _lib.ZS_BF16_SR, **kw)

        sets = {"split_sr": mk16(), "split_sr_again": mk16(), "split_f32": sets["f32"],
                "none_sr": free(half, state_dtype=_lib.ZS_BF16, state_rounding="stochastic"),
                "none_f32": free(rows)}
    elif args.sr:
        sets.update(bf16=mk16(), bf16_again=mk16(), bf16_sr=mk16())
    else:
        sets.update(f32_again=AdamSet(rows, eng.zdtype, eng.p_dtype), bf16=mk16())
    count = {s: 0 for s in SETTINGS}
    m_base = eng.m.data_ptr()

    def block(s, n):
        ev = []
        for _ in range(n):
            count[s] += 1
            sr_state = s in ("bf16_sr", "split_sr", "split_sr_again", "none_sr")
            h = adam_hparams(1e-3, 0.9, 0.999 if sr_state else 0.95, 1e-8, 0.0, count[s])
            keys = sr_keys(0, count[s]) if sr_state or s == "none_f32" else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if s.startswith("none"):
                sets[s].run_psr(h, m_base, keys, stream)
            elif keys is None:
                sets[s].run(h, stream)
            else:
                sets[s].run_sr(h, m_base, keys, stream)
            e1.record(stream)
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    rounds = {s: [] for s in SETTINGS}
    for s in SETTINGS:  # one untimed round: code load, page tables, clocks
        block(s, args.steps)
    for r in range(args.rounds):
        for s in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
            ms = block(s, args.steps)
            rounds[s].append(float(np.median(ms)))
            print(json.dumps({"round": r, "setting": s, "median_ms": rounds[s][-1],
                              "min_ms": min(ms), "max_ms": max(ms)}), flush=True)
    n_el = int(sum(p.numel() for p in params))
    summary = {"config": f"{args.config} {name}", "params": n_el, "kind": args.kind,
               "rounds": args.rounds, "steps_per_round": args.steps,
               "placement": getattr(eng, "placement", None), "settings": []}
    for s in SETTINGS:
        med = float(np.median(rounds[s]))
        nbytes = sets[s].bytes
        gbs = nbytes / med / 1e6
        summary["settings"].append({
            "setting": s, "round_medians_ms": rounds[s], "median_ms": med,
            "spread_ms": max(rounds[s]) - min(rounds[s]), "bytes": int(nbytes),
            "bytes_per_element": nbytes / n_el, "gbs": gbs, "frac_of_8tbs": gbs / PEAK_GBS,
            "frac_round_min_max": [nbytes / m / 1e6 / PEAK_GBS
                                   for m in (max(rounds[s]), min(rounds[s]))]})
    if args.psr:
        by = {x["setting"]: x for x in summary["settings"]}
        same = [abs(a - b) for a, b in zip(rounds["split_sr"], rounds["split_sr_again"])]
        split_ms = float(np.median(rounds["split_sr"] + rounds["split_sr_again"]))
        gain_sr = [min(a, b) - c for a, b, c in zip(rounds["split_sr"], rounds["split_sr_again"],
                                                    rounds["none_sr"])]
        gain_f32 = [a - c for a, c in zip(rounds["split_f32"], rounds["none_f32"])]
        summary["verdict"] = {
            "split_vs_split_abs_diff_ms_per_round": same, "ab_spread_ms": max(same),
            "spread_over_split": max(same) / split_ms,
            "none_sr_gain_ms_per_round": gain_sr, "none_f32_gain_ms_per_round": gain_f32,
            "none_sr_faster_in_every_round_by_more_than_the_spread": bool(min(gain_sr) > max(same)),
            "none_f32_faster_in_every_round_by_more_than_the_spread": bool(min(gain_f32) > max(same)),
            "time_ratio_none_sr_over_split_sr": by["none_sr"]["median_ms"] / split_ms,
            "bytes_ratio_none_sr_over_split_sr": by["none_sr"]["bytes"] / by["split_sr"]["bytes"],
            "time_ratio_none_f32_over_split_f32":
                by["none_f32"]["median_ms"] / by["split_f32"]["median_ms"],
            "bytes_ratio_none_f32_over_split_f32": by["none_f32"]["bytes"] / by["split_f32"]["bytes"]}
        print(json.dumps(summary), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
        dist.destroy_process_group()
        return
    if args.sr:
        by = {x["setting"]: x for x in summary["settings"]}
        same = [abs(a - b) for a, b in zip(rounds["bf16"], rounds["bf16_again"])]
        near_ms = float(np.median(rounds["bf16"] + rounds["bf16_again"]))
        over = [c - max(a, b) for a, b, c in zip(rounds["bf16"], rounds["bf16_again"], rounds["bf16_sr"])]
        summary["verdict"] = {
            "nearest_vs_nearest_abs_diff_ms_per_round": same, "ab_spread_ms": max(same),
            "sr_minus_slower_nearest_ms_per_round": over,
            "sr_slower_than_nearest_by_more_than_the_spread": bool(max(over) > max(same)),
            "sr_faster_than_f32_in_every_round": bool(all(
                c < a for a, c in zip(rounds["f32"], rounds["bf16_sr"]))),
            "time_ratio_sr_over_nearest": by["bf16_sr"]["median_ms"] / near_ms,
            "spread_over_nearest": max(same) / near_ms,
            "time_ratio_sr_over_f32": by["bf16_sr"]["median_ms"] / by["f32"]["median_ms"],
            "bytes_ratio_sr_over_nearest": by["bf16_sr"]["bytes"] / by["bf16"]["bytes"]}
        print(json.dumps(summary), flush=True)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
        dist.destroy_process_group()
        return
    same = [abs(a - b) for a, b in zip(rounds["f32"], rounds["f32_again"])]
    gain = [min(a, b) - c for a, b, c in zip(rounds["f32"], rounds["f32_again"], rounds["bf16"])]
    f32_ms = float(np.median(rounds["f32"] + rounds["f32_again"]))
    b16 = summary["settings"][2]
    summary["verdict"] = {
        "f32_vs_f32_abs_diff_ms_per_round": same, "ab_spread_ms": max(same),
        "bf16_gain_ms_per_round": gain, "min_gain_ms": min(gain),
        "bf16_faster_in_every_round_by_more_than_the_spread": bool(min(gain) > max(same)),
        "time_ratio_bf16_over_f32": b16["median_ms"] / f32_ms,
        "bytes_ratio_bf16_over_f32": b16["bytes"] / summary["settings"][0]["bytes"]}
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
