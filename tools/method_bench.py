#!/usr/bin/env python3
"""Training-step time (forward + adjoint backward + Adam) of ODEGCN3 under the fixed-grid methods rk4 / midpoint / euler
at step_size 1/16, in one process with the methods alternating round by round; the median of the rounds is reported.

  cora   Cora, hidden 16: the native / captured path (one C call per solve, replayed as a HIP graph from the second
         request on) beside the per-stage Python driver (odeint.NATIVE_RK4 = False, capture off)
  rmat   an R-MAT graph of 2^scale nodes (default 17, 16 edges per node) at d = 128: the large route

The expectation to confirm or refute: per function evaluation the methods cost the same, so at the large size a step costs
about S / 4 of rk4's (S = 4, 2, 1 stages), and at Cora's size the same holds once the solve is native or replayed.
Prints one JSON line.

  python tools/method_bench.py [--rounds 3] [--steps 20] [--scale 17] [--no-cora] [--no-rmat]
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
from graph_odenet_amd import models, odeint as OI  # noqa: E402
from graph_odenet_amd.optim import Adam  # noqa: E402
from graph_odenet_amd.solver import n_stages  # noqa: E402

METHODS = ("rk4", "midpoint", "euler")


def cora(dev):
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "cora_graph.npz")))
    n = int(g["n"])
    T = lambda a: torch.from_numpy(np.asarray(a))   # noqa: E731
    adj = torch.sparse_coo_tensor(torch.stack([T(g["rows"].astype(np.int64)), T(g["cols"].astype(np.int64))]),
                                  T(g["vals"]), (n, n))
    x = torch.zeros(n, int(g["n_feat"]))
    x[T(g["feat_rows"].astype(np.int64)), T(g["feat_cols"].astype(np.int64))] = T(g["feat_vals"])
    idx = T(g["idx_train"].astype(np.int64))
    return adj.to(dev), x.to(dev), T(g["labels"].astype(np.int64)).to(dev), idx.to(dev)


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
        med = float(np.median(v))
        nfe = 2 * 16 * n_stages(m)                  # forward + adjoint solve, 16 steps each
        out[m] = {"step_ms": round(med, 3), "step_ms_all": [round(a, 3) for a in v], "solve_evals": nfe}
    for m in METHODS:
        out[m]["vs_rk4"] = round(out[m]["step_ms"] / out["rk4"]["step_ms"], 3)
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
    out = {"metric": "ODEGCN3 fwd + adjoint bwd + Adam, ms per step, fixed grid of 16 steps", "methods": list(METHODS)}
    if not args.no_cora:
        adj, x, labels, idx = cora(dev)

        def make(method):
            torch.manual_seed(0)
            return models.ODEGCN3(nfeat=x.shape[1], nhid=16, nclass=7, dropout=0.5, method=method, step_size=1 / 16).to(dev)
        out["cora_native_captured"] = alternate(make, x, adj, labels, idx, args.steps, args.rounds, 5)
        native, cap = OI.NATIVE_RK4, OI.GRAPH_CAPTURE_MAX_ELEMS
        OI.NATIVE_RK4, OI.GRAPH_CAPTURE_MAX_ELEMS = False, 0
        try:
            out["cora_per_stage"] = alternate(make, x, adj, labels, idx, args.steps, args.rounds, 5)
        finally:
            OI.NATIVE_RK4, OI.GRAPH_CAPTURE_MAX_ELEMS = native, cap
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
            return models.ODEGCN3(nfeat=128, nhid=128, nclass=16, dropout=0.5, method=method, step_size=1 / 16).to(dev)
        out["rmat"] = dict(nodes=n, edges=16 << args.scale, hidden=128,
                           **alternate(make_big, x, g, labels, idx, max(args.steps // 5, 2), args.rounds, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
