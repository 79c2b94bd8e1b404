"""How far bf16 Adam moments move a short run from the fp32-moment one, on the CPU through the
oracles (no GPU): the 10-step D = 64 reference trajectory (tests/golden/traj_z2_ws2_d64_ref.npz: the
harness MLP, its inputs and initial parameters; gradients from oracle/zero_oracle.py mlp_grads on
the run's own parameters, averaged over the two ranks) with Adam(lr, betas=(0.9, beta2)), once with
fp32 moments and once with the moments widened, updated by the same ``adam_update`` and rounded to
bf16 (nearest even) after every step.  Prints, per step, the normwise relative deviation of all
parameters, || p_bf16 - p_fp32 || / || p_fp32 ||, and the same against the distance the fp32 run
has moved from the initial parameters.

``--master-free``: the loss curve of the same model with bf16 parameters, once under the split
master (an fp32 master whose bf16 rounding the model computes with) and once with ``master="none"``
(the bf16 parameter alone, stored with the stochastic rounding of tests/_psr_oracle.py, element i
of parameter k at shard index offset_k + i, seed ``--seed``), fp32 moments in both; per step the
two losses and their relative difference.  A recorded result, not a check.

Usage: python tools/bf16_state_closeness.py [--beta2 0.95] [--lr 1e-3] [--master-free] [--seed 0]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

from oracle import zero_oracle as zo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beta2", type=float, default=0.95)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--master-free", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    z = np.load(REPO / "tests" / "golden" / "traj_z2_ws2_d64_ref.npz")
    ws, steps = int(z["ws"]), int(z["steps"])
    init = [z[f"init_{i}"].astype(np.float32) for i in range(12)]
    xs = [z["x"] if "x" in z.files else z[f"r{r}_x"] for r in range(ws)]
    ys = [z["y"] if "y" in z.files else z[f"r{r}_y"] for r in range(ws)]
    widen = lambda b: zo.bf16_bits_to_f32(b).reshape(b.shape)  # noqa: E731
    narrow = lambda x: zo.f32_to_bf16_bits(x).reshape(x.shape)  # noqa: E731
    flat = lambda ps: np.concatenate([p.reshape(-1).astype(np.float64) for p in ps])  # noqa: E731
    if args.master_free:
        return master_free_leg(args, init, xs, ys, ws, steps, widen, narrow)
    runs = {}
    for name in ("fp32", "bf16"):
        p = [a.copy() for a in init]
        m = [np.zeros_like(a) for a in init]
        v = [np.zeros_like(a) for a in init]
        traj = []
        for t in range(1, steps + 1):
            per_rank = [zo.mlp_grads(p, xs[r], ys[r])[1] for r in range(ws)]
            for i in range(12):
                g = (sum(gr[i].astype(np.float32) for gr in per_rank) / np.float32(ws)).astype(np.float32)
                p[i], m[i], v[i], _ = zo.adam_update(p[i], g, m[i], v[i], t, lr=args.lr,
                                                     betas=(0.9, args.beta2))[:4]
                if name == "bf16":
                    m[i], v[i] = widen(narrow(m[i])), widen(narrow(v[i]))
            traj.append(flat(p))
        runs[name] = traj
    p0 = flat(init)
    rows = []
    for t, (a, b) in enumerate(zip(runs["fp32"], runs["bf16"]), 1):
        d = float(np.linalg.norm(b - a))
        rows.append({"step": t, "rel_to_params": d / float(np.linalg.norm(a)),
                     "rel_to_distance_moved": d / float(np.linalg.norm(a - p0))})
        print(json.dumps(rows[-1]))
    print(json.dumps({"beta2": args.beta2, "lr": args.lr, "steps": steps,
                      "max_rel_to_params": max(r["rel_to_params"] for r in rows),
                      "max_rel_to_distance_moved": max(r["rel_to_distance_moved"] for r in rows)}))


def master_free_leg(args, init, xs, ys, ws, steps, widen, narrow):
    sys.path.insert(0, str(REPO / "tests"))
    import _psr_oracle as po

    offs = np.concatenate([[0], np.cumsum([a.size for a in init])]).astype(np.uint64)
    curves = {}
    for name in ("split", "none"):
        master = [widen(narrow(a)) for a in init]  # both start from the same bf16 parameters
        m = [np.zeros_like(a) for a in init]
        v = [np.zeros_like(a) for a in init]
        losses = []
        for t in range(1, steps + 1):
            model = [widen(narrow(a)) for a in master]  # what the forward and backward see
            out = [zo.mlp_grads(model, xs[r], ys[r]) for r in range(ws)]
            losses.append(float(np.mean([o[0] for o in out])))
            keys = po.keys_of(args.seed, t)
            for i in range(12):
                g = (sum(o[1][i].astype(np.float32) for o in out) / np.float32(ws)).astype(np.float32)
                g = widen(narrow(g))  # bf16 gradients, as the bf16 model hands them over
                src = master[i] if name == "split" else model[i]
                p, m[i], v[i], _ = zo.adam_update(src, g, m[i], v[i], t, lr=args.lr,
                                                  betas=(0.9, args.beta2))[:4]
                if name == "none":
                    e = offs[i] + np.arange(p.size, dtype=np.uint64)
                    p = widen(po.narrow_param(p.reshape(-1), e, keys)).reshape(p.shape)
                master[i] = p
        curves[name] = losses
    for t, (a, b) in enumerate(zip(curves["split"], curves["none"]), 1):
        print(json.dumps({"step": t, "loss_split": a, "loss_none": b, "rel_diff": (b - a) / a}))
    print(json.dumps({"beta2": args.beta2, "lr": args.lr, "steps": steps, "seed": args.seed,
                      "final_loss_split": curves["split"][-1], "final_loss_none": curves["none"][-1],
                      "max_abs_rel_diff": max(abs(b - a) / a for a, b in
                                              zip(curves["split"], curves["none"]))}))


if __name__ == "__main__":
    main()
