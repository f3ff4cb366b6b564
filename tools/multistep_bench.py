#!/usr/bin/env python3
"""Training-step time (forward + adjoint backward + Adam) of ODEGCN3 at step_size 1/16 under rk4, explicit_adams, midpoint and
euler, in one process with the methods alternating round by round; the median of the rounds is reported (the manner of
tools/method_bench.py, whose Cora loader is used).

  cora   Cora, hidden 16: the native path, replayed as a HIP graph from the second request on
  rmat   an R-MAT graph of 2^scale nodes (default 17, 16 edges per node) at d = 128: the large route (forward solve native,
         adjoint solve through solver.integrate_multistep / integrate_fixed)

The expectation, written down before the first run (README.md, Methods):
  * the solve part of a step scales with the evaluations, forward + adjoint: explicit_adams 25 + 26 against rk4's 64 + 65,
    midpoint's 32 + 33, euler's 16 + 17 - so explicit_adams should sit between midpoint and euler, nearer midpoint's 0.5 x rk4
    than 51 / 129 = 0.40 x by what does not scale: the two plain layers, the loss, Adam, one replay's fixed cost;
  * on the large route a multistep evaluation costs a little more than an rk4 stage: its closing SpMM reads four `pre` terms
    and stores K, and on the adjoint side the Python driver closes a step with a 5-term lincomb per component group where
    rk4's last stage folds the combination into the producing launches.
Prints one JSON line.

  python tools/multistep_bench.py [--rounds 3] [--steps 20] [--scale 17] [--no-cora] [--no-rmat]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from graph_odenet_amd import models, odeint as OI  # noqa: E402
from graph_odenet_amd.optim import Adam  # noqa: E402
from method_bench import cora  # noqa: E402

METHODS = ("rk4", "explicit_adams", "midpoint", "euler")
GRID = 16


def alternate(make, x, graph, labels, idx, steps, rounds, warmup):
    """{method: figures} with one model per method (the same seed) taking turns round by round."""
    runs = {}
    for m in METHODS:
        model = make(m)
        runs[m] = (model, Adam(model.parameters(), lr=0.01, weight_decay=5e-4))

    def step(model, opt):
        opt.zero_grad(set_to_none=False)
        out = model(x, graph)
        torch.nn.functional.nll_loss(out[idx], labels[idx]).backward()
        opt.step()
    res = {m: [] for m in METHODS}
    for r in range(rounds):
        for m in METHODS:
            for _ in range(warmup if r == 0 else 1):
                step(*runs[m])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(*runs[m])
            torch.cuda.synchronize()
            res[m].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {}
    for m, v in res.items():
        nfe = OI._grid_nfe(m, GRID)
        out[m] = {"step_ms": round(float(np.median(v)), 3), "step_ms_all": [round(a, 3) for a in v],
                  "solve_evals": [nfe, nfe + 1]}                 # forward, adjoint (with the counted dL/dt evaluation)
    for m in METHODS:
        out[m]["vs_rk4"] = round(out[m]["step_ms"] / out["rk4"]["step_ms"], 3)
        out[m]["evals_vs_rk4"] = round(sum(out[m]["solve_evals"]) / sum(out["rk4"]["solve_evals"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="timed training steps per round on Cora (R-MAT: a fifth)")
    ap.add_argument("--scale", type=int, default=17)
    ap.add_argument("--no-cora", action="store_true")
    ap.add_argument("--no-rmat", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "ODEGCN3 fwd + adjoint bwd + Adam, ms per step, fixed grid of %d steps" % GRID, "methods": list(METHODS)}
    if not args.no_cora:
        adj, x, labels, idx = cora(dev)

        def make(method):
            torch.manual_seed(0)
            return models.ODEGCN3(nfeat=x.shape[1], nhid=16, nclass=7, dropout=0.5, method=method, step_size=1 / GRID).to(dev)
        out["cora_native_captured"] = alternate(make, x, adj, labels, idx, args.steps, args.rounds, 5)
        del adj, x
    if not args.no_rmat:
        from graph_odenet_amd.synth import rmat_graph
        g = rmat_graph(args.scale, 16 << args.scale, seed=0, device=dev)
        g.transpose()
        n = g.n_rows
        gen = torch.Generator(device=dev).manual_seed(1000)
        x = torch.randn(n, 128, generator=gen, device=dev)
        labels = torch.randint(0, 16, (n,), generator=gen, device=dev)
        idx = torch.randperm(n, generator=gen, device=dev)[: n // 10]

        def make_big(method):
            torch.manual_seed(42)
            return models.ODEGCN3(nfeat=128, nhid=128, nclass=16, dropout=0.5, method=method, step_size=1 / GRID).to(dev)
        out["rmat"] = dict(nodes=n, edges=16 << args.scale, hidden=128,
                           **alternate(make_big, x, g, labels, idx, max(args.steps // 5, 2), args.rounds, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
