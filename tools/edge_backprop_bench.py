#!/usr/bin/env python3
"""Training-step time of the QM9 edge-conditioned ODE model under the three ways its block gets gradients, in one process
with the modes taking turns round by round: the adjoint solve (adjoint=True), backprop through the solve on the fused
sweep (adjoint=False; qc_ode.EdgeOdeField, csrc/edge_backprop.hip) and backprop through the solve on the generic path
(EdgeOdeField.BACKPROP_FUSED = False: every interval re-run as torch ops under autograd).  EdgeODE1_K_Sum, hidden 96,
fwd + bwd + Adam, a new batch of 20 QM9-like molecules every step (the same batches for every mode), under rk4 (step
0.25) and under dopri5 (rtol = atol = --tol).  Prints one JSON line: the median ms per step of every mode and round.

  python tools/edge_backprop_bench.py [--steps 30] [--rounds 3] [--warmup 5] [--hidden 96] [--tol 1e-3] [--methods rk4,dopri5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_odenet_amd import qc_models, qc_ode  # noqa: E402
from graph_odenet_amd.optim import Adam  # noqa: E402
from graph_odenet_amd.synth import qm9_like_batch  # noqa: E402

MODES = ("adjoint", "fused", "generic")


def alternate(net, opt, batches, rounds, warmup):
    """{mode: per-round list of the median ms of a step}, the modes taking turns round by round."""

    def step(b):
        x, ef, Esrc, Etgt, batch, tgt = b
        opt.zero_grad(set_to_none=True)
        F.mse_loss(net(x, ef, Esrc, Etgt, batch), tgt).backward()
        opt.step()
    res = {m: [] for m in MODES}
    try:
        for r in range(rounds):
            for mode in MODES:
                net.ode.adjoint = mode == "adjoint"
                qc_ode.EdgeOdeField.BACKPROP_FUSED = mode != "generic"
                for b in (batches if r == 0 else batches[:warmup]):      # round 0: every batch shape once per mode
                    step(b)
                ts = []
                for b in batches:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    step(b)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                res[mode].append(round(float(np.median(ts)), 3))
    finally:
        qc_ode.EdgeOdeField.BACKPROP_FUSED = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps before each later round (round 0: all batches)")
    ap.add_argument("--hidden", type=int, default=96)
    ap.add_argument("--batch-size", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-3, help="rtol = atol of the dopri5 runs")
    ap.add_argument("--methods", default="rk4,dopri5")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = []
    for b in range(args.steps):
        x, ef, Esrc, Etgt, batch = qm9_like_batch(args.batch_size, seed=7000 + b, device=dev)
        tgt = torch.randn(args.batch_size, 12, generator=torch.Generator().manual_seed(b)).to(dev)
        batches.append((x, ef, Esrc, Etgt, batch, tgt))
    out = {"metric": "EdgeODE1_K_Sum fwd+bwd+Adam step, ms (median over the steps of a round), by gradient mode",
           "hidden": args.hidden, "batch_size": args.batch_size, "steps_per_round": args.steps,
           "atoms": int(np.median([b[0].shape[0] for b in batches])), "edges": int(np.median([b[2].numel() for b in batches]))}
    for method in args.methods.split(","):
        kw = dict(method="rk4", step_size=0.25) if method == "rk4" else dict(method=None, tol=args.tol)
        torch.manual_seed(0)
        net = qc_models.EdgeODE1_K_Sum(node_features=13, edge_features=5, target_features=12, hidden_features=args.hidden,
                                       **kw).to(dev)
        per_round = alternate(net, Adam(net.parameters(), lr=1e-3), batches, args.rounds, args.warmup)
        out[method] = dict({m: {"step_ms": round(float(np.median(v)), 3), "step_ms_rounds": v} for m, v in per_round.items()},
                           fused_below_generic_every_round=all(a < b for a, b in zip(per_round["fused"], per_round["generic"])),
                           **({"tol": args.tol} if method != "rk4" else {"step_size": 0.25}))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
