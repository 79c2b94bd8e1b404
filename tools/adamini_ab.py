"""In-process A/B of the fused Adam-mini (csrc/zs_adamini.hip) against its siblings among the
element-wise kernels, on the split master at a benchmark configuration's size (default C4), in the
form of tools/adafactor_ab.py.

ONE process, the same placed buffers (bf16 parameter, int16 residual, bf16 gradient, fp32 exp_avg),
one kernel set per variant over the same parameters, the variants interleaved in every round after
one untimed round, every launch between two HIP events.  Per variant: the median of each round,
their median and the spread (max - min) between rounds.

Variants: Adam-mini with block_rows=1 everywhere at the default resident_cap (``mini``), the same
with resident_cap=0 (``mini_cap0``: every block through the two passes), Adam-mini with
block_rows=128 on the Q and K matrices (``mini_heads``), the two paths of ``mini_heads`` alone
(``heads_resident``, ``heads_twopass``), Adam with fp32 moments (26 B/element), Adam with bf16 moments
(18) and SGD with momentum (18, the resident path's sibling).  Nothing is gated.

Usage: python tools/adamini_ab.py [--rounds 5] [--steps 20] [--config C4] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "distributed-training-sandbox_amd"))

VARIANTS = ("mini", "mini_cap0", "mini_heads", "heads_resident", "heads_twopass", "adam_f32",
            "adam_bf16", "sgd_momentum")


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
    from zero_amd.kernels import (ADAMINI_RESIDENT_CAP, AdamMiniSet, AdamSet, SgdSet, adam_hparams,
                                  adamini_hparams, sgd_hparams)
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
    m32 = torch.zeros(total, dtype=torch.float32, device=dev)
    v32 = torch.zeros(total, dtype=torch.float32, device=dev)
    mb = torch.zeros(total, dtype=torch.bfloat16, device=dev)
    vb = torch.zeros(total, dtype=torch.bfloat16, device=dev)
    # decoder sets: tensors 1 + 9 k and 2 + 9 k are the Q and K matrices (head_dim 128)
    decoder = args.config in ("C4", "C5")
    is_qk = [decoder and len(s) == 2 and i >= 1 and (i - 1) % 9 in (0, 1) for i, s in enumerate(shapes)]

    def mini_set(heads: bool, cap: int):
        brs = [0 if len(s) < 2 else 128 if heads and qk else 1 for s, qk in zip(shapes, is_qk)]
        nblk = [1 if b == 0 else s[0] // b for s, b in zip(shapes, brs)]
        voff = np.concatenate([[0], np.cumsum([(b + 3) // 4 * 4 for b in nblk])])
        vblk = torch.zeros(int(voff[-1]), dtype=torch.float32, device=dev)
        rows = [[g.data_ptr() + 2 * o, hi.data_ptr() + 2 * o, lo.data_ptr() + 2 * o,
                 hi.data_ptr() + 2 * o, m32.data_ptr() + 4 * o, vblk.data_ptr() + 4 * int(vo),
                 1 if len(s) < 2 else s[0], n if len(s) < 2 else n // s[0], b, i]
                for i, (s, n, o, vo, b) in enumerate(zip(shapes, numels, offs, voff, brs))]
        return AdamMiniSet(np.array(rows, np.uint64), BF16, SPLIT, resident_cap=cap), vblk

    def rows(m, v):
        r = np.zeros((len(numels), 9), np.uint64)
        o = np.asarray(offs, np.uint64)
        r[:, 0] = np.uint64(g.data_ptr()) + o * np.uint64(2)
        r[:, 1] = r[:, 3] = np.uint64(hi.data_ptr()) + o * np.uint64(2)
        r[:, 2] = np.uint64(lo.data_ptr()) + o * np.uint64(2)
        r[:, 4] = np.uint64(m.data_ptr()) + o * np.uint64(m.element_size())
        if v is not None:
            r[:, 5] = np.uint64(v.data_ptr()) + o * np.uint64(v.element_size())
        r[:, 8] = np.asarray(numels, np.uint64)
        return r

    BF16, SPLIT = _lib.ZS_BF16, _lib.ZS_BF16_SPLIT
    mini, _v0 = mini_set(False, ADAMINI_RESIDENT_CAP)
    cap0, _v1 = mini_set(False, 0)
    heads, _v2 = mini_set(True, ADAMINI_RESIDENT_CAP)
    adam32 = AdamSet(rows(m32, v32), BF16, SPLIT)
    adam16 = AdamSet(rows(mb, vb), BF16, SPLIT, state_dtype=BF16)
    sgd = SgdSet(rows(m32, None), BF16, SPLIT)
    mhp, shp = adamini_hparams(1e-3), sgd_hparams(1e-3, 0.9)
    st = torch.cuda.current_stream()
    count = {k: 0 for k in VARIANTS}
    nbytes = {"mini": mini.bytes, "mini_cap0": cap0.bytes, "mini_heads": heads.bytes,
              "heads_resident": heads.resident_bytes, "heads_twopass": heads.twopass_bytes,
              "adam_f32": adam32.bytes, "adam_bf16": adam16.bytes, "sgd_momentum": sgd.bytes}

    def launch(k):
        count[k] += 1
        if k in ("mini", "mini_cap0", "mini_heads"):
            {"mini": mini, "mini_cap0": cap0, "mini_heads": heads}[k].run(mhp, count[k], st)
        elif k == "heads_resident":
            heads.run_pass(mhp, 7, 0, st)
        elif k == "heads_twopass":
            heads.run_pass(mhp, 7, 1, st)
            heads.run_pass(mhp, 7, 2, st)
        elif k == "sgd_momentum":
            sgd.run(shp, st)
        else:  # (beta2 0.99: within the bound of bf16 moments rounded to nearest)
            (adam32 if k == "adam_f32" else adam16).run(
                adam_hparams(1e-3, 0.9, 0.99, 1e-8, 0.0, count[k]), st)

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
               "resident_cap": ADAMINI_RESIDENT_CAP,
               "sets": {k: {"blocks": s.blocks, "resident_elems": s.resident_elems,
                            "twopass_elems": s.twopass_elems, "scratch_bytes": s.scratch_bytes,
                            "block_state_bytes_per_param": 4 * s.blocks / elems}
                        for k, s in (("mini", mini), ("mini_cap0", cap0), ("mini_heads", heads))},
               "variants": {}}
    for k in VARIANTS:
        med = float(np.median(rounds[k]))
        summary["variants"][k] = {"round_medians_ms": rounds[k], "median_ms": med,
                                  "spread_ms": max(rounds[k]) - min(rounds[k]),
                                  "bytes_per_element": nbytes[k] / elems,
                                  "gbs": nbytes[k] / med / 1e6}
    vs = summary["variants"]
    gap = vs["mini_cap0"]["median_ms"] - vs["mini"]["median_ms"]
    summary["resident_minus_cap0_ms"] = -gap
    summary["resident_wins"] = bool(gap > max(vs["mini"]["spread_ms"], vs["mini_cap0"]["spread_ms"]))
    print(json.dumps(summary), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")


if __name__ == "__main__":
    main()
