"""In-process A/B of the fused Adafactor's three passes against their siblings among the
element-wise kernels, on the split master at a benchmark configuration's size (default C4).

Placement differs from process to process, so everything is judged here: ONE process, the same
placed buffers (bf16 parameter, int16 residual, bf16 gradient), one kernel set per variant over the
same parameters, stepped in alternating blocks, every launch between two HIP events, one untimed
round first.  Per variant: the median of each round, their median and the spread (max - min)
between rounds.

Siblings: the gradient-norm pass is read-only like pass B (2 B/element); the momentum-free SGD
instance moves pass C's 10 B/element; Adam with bf16 moments moves the whole step's 18 B/element.
Nothing is gated: the rates are recorded side by side.

Usage: python tools/adafactor_ab.py [--rounds 5] [--steps 20] [--config C4] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))

VARIANTS = ("pass_a", "pass_b", "pass_c", "adafactor", "grad_norm", "sgd_plain", "adam_bf16")


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
    from zero_amd.flat import AdafactorState
    from zero_amd.kernels import (AdafactorSet, AdamSet, SgdSet, adafactor_hparams, adam_hparams,
                                  sgd_hparams)
    from zero_amd.shapes import CONFIGS

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    name, shape_fn = CONFIGS[args.config]
    shapes = [tuple(int(x) for x in s) for s in shape_fn()]
    numels = [int(np.prod(s, dtype=np.int64)) for s in shapes]
    offs, total = [], 0
    for n in numels:  # every parameter 256-byte aligned in every array
        offs.append(total)
        total += (n + 127) // 128 * 128
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    hi = torch.empty(total, dtype=torch.float32, device=dev).normal_(0.0, 0.02, generator=gen).to(
        torch.bfloat16)
    lo = torch.zeros(total, dtype=torch.int16, device=dev)
    g = (torch.empty(total, dtype=torch.float32, device=dev).normal_(generator=gen) * 1e-3).to(
        torch.bfloat16)
    m = torch.zeros(total, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(total, dtype=torch.bfloat16, device=dev)
    soff, stotal = [], 0
    for s in shapes:
        cur = []
        for n in AdafactorState.sizes(s):
            cur.append(stotal)
            stotal += (n + 3) // 4 * 4
        soff.append(cur)
    factors = torch.zeros(stotal, dtype=torch.float32, device=dev)

    def rows(state):
        r = np.zeros((len(numels), 9), np.uint64)
        o = np.asarray(offs, np.uint64)
        r[:, 0] = np.uint64(g.data_ptr()) + o * np.uint64(2)
        r[:, 1] = r[:, 3] = np.uint64(hi.data_ptr()) + o * np.uint64(2)
        r[:, 2] = np.uint64(lo.data_ptr()) + o * np.uint64(2)
        if state:
            r[:, 4] = np.uint64(m.data_ptr()) + o * np.uint64(2)
            r[:, 5] = np.uint64(v.data_ptr()) + o * np.uint64(2)
        r[:, 8] = np.asarray(numels, np.uint64)
        return r

    af_rows = []
    for i, (s, o) in enumerate(zip(shapes, offs)):
        oned = len(s) < 2
        R, C = (1, numels[i]) if oned else s[-2:]
        for b in range(1 if oned else int(np.prod(s[:-2], dtype=np.int64))):
            e = 2 * (o + b * R * C)
            af_rows.append([g.data_ptr() + e, hi.data_ptr() + e, lo.data_ptr() + e, hi.data_ptr() + e,
                            factors.data_ptr() + 4 * (soff[i][0] + b * R),
                            0 if oned else factors.data_ptr() + 4 * (soff[i][1] + b * C), R, C, i])
    BF16, SPLIT = _lib.ZS_BF16, _lib.ZS_BF16_SPLIT
    af = AdafactorSet(np.array(af_rows, np.uint64), BF16, SPLIT)
    sgd = SgdSet(rows(False), BF16, SPLIT)
    adam = AdamSet(rows(True), BF16, SPLIT, state_dtype=BF16)
    partials = torch.zeros(sgd.sqnorm_partials, dtype=torch.float64, device=dev)
    ahp = adafactor_hparams(1e-2)
    shp = sgd_hparams(1e-3, 0.0)
    st = torch.cuda.current_stream()
    count = {k: 0 for k in VARIANTS}
    nbytes = {"pass_a": af.pass_bytes[0], "pass_b": af.pass_bytes[1], "pass_c": af.pass_bytes[2],
              "adafactor": af.bytes, "grad_norm": sgd.grad_bytes, "sgd_plain": sgd.bytes,
              "adam_bf16": adam.bytes}

    def launch(k):
        count[k] += 1
        if k.startswith("pass_"):
            af.run_pass(ahp, 7, "abc".index(k[-1]), st)
        elif k == "adafactor":
            af.run(ahp, count[k], st)
        elif k == "grad_norm":
            sgd.grad_sqnorm(partials, st)
        elif k == "sgd_plain":
            sgd.run(shp, st)
        else:  # (beta2 0.99: within the bound of bf16 moments rounded to nearest)
            adam.run(adam_hparams(1e-3, 0.9, 0.99, 1e-8, 0.0, count[k]), st)

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
    af.run(ahp, 1, st)  # (the single passes need the factors and scalars of a whole step)
    for k in VARIANTS:  # one untimed round: code load, page tables, clocks
        block(k, args.steps)
    for r in range(args.rounds):
        for k in (VARIANTS if r % 2 == 0 else VARIANTS[::-1]):
            ms = block(k, args.steps)
            rounds[k].append(float(np.median(ms)))
            print(json.dumps({"round": r, "variant": k, "median_ms": rounds[k][-1], "min_ms": min(ms),
                              "max_ms": max(ms), "gbs": nbytes[k] / rounds[k][-1] / 1e6}), flush=True)
    elems = int(sum(numels))
    summary = {"config": f"{args.config} {name}", "params": elems, "master": "split",
               "rounds": args.rounds, "steps_per_round": args.steps,
               "factor_state_bytes": stotal * 4, "factor_state_bytes_per_param": stotal * 4 / elems,
               "scratch_bytes": af.scratch_bytes, "variants": {}}
    for k in VARIANTS:
        med = float(np.median(rounds[k]))
        summary["variants"][k] = {"round_medians_ms": rounds[k], "median_ms": med,
                                  "round_gbs": [nbytes[k] / x / 1e6 for x in rounds[k]],
                                  "spread_ms": max(rounds[k]) - min(rounds[k]),
                                  "bytes_per_element": nbytes[k] / elems,
                                  "gbs": nbytes[k] / med / 1e6}
    vs = summary["variants"]
    summary["rate_vs_sibling"] = {
        "pass_b_over_grad_norm": vs["pass_b"]["gbs"] / vs["grad_norm"]["gbs"],
        "pass_c_over_sgd_plain": vs["pass_c"]["gbs"] / vs["sgd_plain"]["gbs"],
        "adafactor_over_adam_bf16": vs["adafactor"]["gbs"] / vs["adam_bf16"]["gbs"],
        "pass_a_over_adam_bf16": vs["pass_a"]["gbs"] / vs["adam_bf16"]["gbs"]}
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
