#!/usr/bin/env python3
"""Training-step time of odeint_adjoint against odeint backprop (odeint._OdeintBackprop), in one process with the two
modes alternating: ODEGCN3 fwd + bwd + Adam on the C5 graph (R-MAT 2^20 nodes, 10^7 edges, d = 128, rk4 16 steps) and on
Cora (d = 16, rk4 step 1/16), plus each mode's peak device memory.  Prints one JSON line.
--method dopri5: the adaptive default instead (the same Function, its dopri5 strategy), rtol = atol = --tol.

  python tools/backprop_bench.py [--steps 3] [--rounds 3] [--scale 20] [--edges 10000000] [--no-cora] [--only MODE]
                                 [--method rk4|dopri5] [--tol 1e-5]
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
from graph_odenet_amd import models  # noqa: E402
from graph_odenet_amd.optim import Adam  # noqa: E402


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


def alternate(model, opt, x, graph, labels, idx, steps, rounds, warmup, modes=("adjoint", "backprop")):
    """{mode: (median ms per step over the rounds, peak MiB)} with the two modes taking turns round by round."""
    blocks = [m for m in model.modules() if isinstance(m, models.ODEBlock)]

    def step():
        opt.zero_grad(set_to_none=False)
        out = model(x, graph)
        torch.nn.functional.nll_loss(out[idx], labels[idx]).backward()
        opt.step()
    res = {m: [] for m in modes}
    peak = {m: 0 for m in modes}
    for r in range(rounds):
        for mode in modes:
            for b in blocks:
                b.adjoint = mode == "adjoint"
            for _ in range(warmup if r == 0 else 1):
                step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            res[mode].append((time.perf_counter() - t0) * 1e3 / steps)
            peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated() / 2 ** 20)
    return {m: {"step_ms": round(float(np.median(v)), 3), "step_ms_all": [round(a, 3) for a in v],
                "peak_mib": round(peak[m], 1)} for m, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--ode-steps", type=int, default=16)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--no-cora", action="store_true")
    ap.add_argument("--only", choices=["adjoint", "backprop"], default=None, help="time one mode (kernel profiles)")
    ap.add_argument("--method", choices=["rk4", "dopri5"], default="rk4")
    ap.add_argument("--tol", type=float, default=1e-5, help="rtol = atol of --method dopri5 (the reference's 1e-5)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    modes = (args.only,) if args.only else ("adjoint", "backprop")
    out = {"metric": "odeint backprop vs odeint_adjoint, ODEGCN3 fwd+bwd+Adam step", "method": args.method}
    if args.method == "rk4":
        ode = lambda steps: dict(method="rk4", step_size=1.0 / steps)       # noqa: E731
        tag = lambda steps: dict(rk4_steps=steps)                           # noqa: E731
    else:
        ode = lambda steps: dict(method=None, tol=args.tol)                 # noqa: E731
        tag = lambda steps: dict(tol=args.tol)                              # noqa: E731
    if not args.no_c5:
        from graph_odenet_amd.synth import rmat_graph
        g = rmat_graph(args.scale, args.edges, seed=0, device=dev)
        g.transpose()
        n = g.n_rows
        gen = torch.Generator(device=dev).manual_seed(1000)
        x = torch.randn(n, 128, generator=gen, device=dev)
        labels = torch.randint(0, 16, (n,), generator=gen, device=dev)
        idx = torch.randperm(n, generator=gen, device=dev)[: n // 10]
        torch.manual_seed(42)
        m = models.ODEGCN3(nfeat=128, nhid=args.hidden, nclass=16, dropout=0.5, **ode(args.ode_steps)).to(dev)
        out["c5"] = dict(nodes=n, hidden=args.hidden, **tag(args.ode_steps),
                         **alternate(m, Adam(m.parameters(), lr=0.01, weight_decay=5e-4), x, g, labels, idx,
                                     args.steps, args.rounds, args.warmup, modes))
        del m, g, x
        torch.cuda.empty_cache()
    if not args.no_cora:
        adj, x, labels, idx = cora(dev)
        torch.manual_seed(0)
        m = models.ODEGCN3(nfeat=x.shape[1], nhid=16, nclass=7, dropout=0.5, **ode(16)).to(dev)
        out["cora"] = dict(hidden=16, **tag(16),
                           **alternate(m, Adam(m.parameters(), lr=0.01, weight_decay=5e-4), x, adj, labels, idx,
                                       20, args.rounds, 5, modes))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
