#!/usr/bin/env python3
"""The adaptive methods on the GAT and the edge-conditioned (QC) ODE functions: ms per training step and evaluations.

  gat   ODEBlock over the GAT ODE function on the Citeseer edge list (3 327 nodes), one head x 16 and 8 heads x 8, random
        node states, a linear read-out, cross-entropy on 120 nodes, fwd + bwd + Adam; dopri5 / bosh3 / adaptive_heun at
        rtol = atol = 1e-3 and 1e-5, through the adjoint solve (adjoint=True) and through backprop (adjoint=False).  The six
        (method, mode) pairs of a (width, tolerance) take turns, one round = each once; the figure is the median of the rounds.
  step  one attempted adjoint step on the one-head function: gode_gat_ode_dopri5_step_adjoint against
        gode_gat_ode_adaptive_step_adjoint(GODE_RKA_DOPRI5) with `parts` (one closing launch for the six stages) - skipped on
        a tree without the latter.
  qc    tools/edge_backprop_bench.py's model (EdgeODE1_K_Sum, hidden 96, batches of 20 molecules) under bosh3 at 1e-3: the
        adjoint solve, backprop on the fused sweep, backprop on the generic path (on a tree whose field has no bosh3 sweep
        "fused" is the generic path too).

`python tools/gat_adaptive_bench.py [--rounds 3] [--steps 5] [--only gat,step,qc]` prints a table and one JSON line.  The tool
uses nothing a tree without the tableau-driven GAT drivers lacks, so the same file measures both."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.environ.get("GODE_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
METHODS = ("dopri5", "bosh3", "adaptive_heun")
TOLS = (1e-3, 1e-5)
WIDTHS = (("1x16", 16, 1), ("8x8", 64, 8))


def citeseer(dev):
    g = dict(np.load(os.path.join(GOLD, "citeseer_gat_edges.npz")))
    n = int(g["n"])
    src, tgt = torch.from_numpy(g["src"].astype(np.int64)).to(dev), torch.from_numpy(g["tgt"].astype(np.int64)).to(dev)
    e = src.numel()
    Mtgt = torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(e, device=dev)]), torch.ones(e, device=dev), (n, e))
    return n, (src, tgt, Mtgt)


def gat_trainer(dev, n, graph, d, H, method, tol, adjoint):
    from graph_odenet_amd import gat_heads, gat_models, gat_ode
    from graph_odenet_amd.models import ODEBlock
    gat_ode.GatOdeField.ADAPTIVE_NATIVE = True           # the opt-in this tool measures (no effect on a tree without it)
    from graph_odenet_amd.optim import Adam
    torch.manual_seed(0)
    f = gat_models.ODEfunc(d) if H == 1 else gat_heads.ODEfunc(d, H)
    blk = ODEBlock(f, tol=tol, method=method, adjoint=adjoint).to(dev)
    head = torch.nn.Linear(d, 6).to(dev)
    gen = torch.Generator().manual_seed(1)
    x = (0.5 * torch.randn(n, d, generator=gen)).to(dev)
    y, idx = torch.randint(0, 6, (n,), generator=gen).to(dev), torch.arange(120, device=dev)
    opt = Adam(list(blk.parameters()) + list(head.parameters()), lr=0.01)

    def step():
        opt.zero_grad(); blk.nfe = 0
        out = head(blk(x, *graph))
        nf = blk.nfe; blk.nfe = 0
        F.cross_entropy(out[idx], y[idx]).backward(); opt.step()
        return nf, blk.nfe
    return step


def time_gat(dev, n, graph, d, H, tol, rounds, steps, warm=3):
    keys = [(m, a) for m in METHODS for a in (True, False)]
    fns = {k: gat_trainer(dev, n, graph, d, H, k[0], tol, k[1]) for k in keys}
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ms, nfe = {k: [] for k in keys}, {}
    for _ in range(rounds):
        for k in keys:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                nfe[k] = fns[k]()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
    return {k: (sorted(ms[k])[len(ms[k]) // 2],) + tuple(nfe[k]) for k in keys}


def time_adjoint_step(dev, n, graph, reps=50):
    """ms per attempted adjoint step (host time around `reps` calls, each ending in the driver's own device->host read of the
    error sums as in a solve): the dopri5 driver and the tableau-driven one on GODE_RKA_DOPRI5 with parts; 3 turns, median."""
    from graph_odenet_amd import gat_models, gat_ode, solver
    gat_ode.GatOdeField.ADAPTIVE_NATIVE = True
    torch.manual_seed(0)
    f = gat_models.ODEfunc(16).to(dev)
    f.set_adj(*graph)
    x0 = (0.5 * torch.randn(n, 16, generator=torch.Generator().manual_seed(1))).to(dev)
    _, mk_adj, _ = f.gode_fields(x0)
    adj = mk_adj()
    adj.prepare()
    if getattr(adj, "adaptive_step_native", None) is None:
        return None
    y = adj.new_state(x0)
    y[1].copy_(torch.randn(n, 16, generator=torch.Generator().manual_seed(2)).to(dev))
    kk = solver._alloc_like(y, 7)
    (y1,) = solver._alloc_like(y, 1)
    adj.eval(0.25, [[(1.0, c)] for c in y], kk[0])
    assert adj._adjoint_parts(7) is not None
    calls = {"dopri5_driver": lambda: adj.dopri5_step_native(y, kk, y1, 0.25, -0.3, 1e-3, 1e-3).tolist(),
             "adaptive_driver_parts": lambda: adj.adaptive_step_native("dopri5", y, kk, y1, 0.25, -0.3, 1e-3, 1e-3).tolist()}
    res = {k: [] for k in calls}
    for _ in range(3):
        for k, fn in calls.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            res[k].append(1e3 * (time.perf_counter() - t0) / reps)
    return {k: round(sorted(v)[1], 4) for k, v in res.items()}


def time_qc(dev, rounds, steps, hidden=96, tol=1e-3):
    import edge_backprop_bench as EB
    from graph_odenet_amd import qc_models
    from graph_odenet_amd.optim import Adam
    from graph_odenet_amd.synth import qm9_like_batch
    batches = []
    for b in range(steps):
        x, ef, Esrc, Etgt, batch = qm9_like_batch(20, seed=7000 + b, device=dev)
        batches.append((x, ef, Esrc, Etgt, batch, torch.randn(20, 12, generator=torch.Generator().manual_seed(b)).to(dev)))
    torch.manual_seed(0)
    net = qc_models.EdgeODE1_K_Sum(node_features=13, edge_features=5, target_features=12, hidden_features=hidden,
                                   method="bosh3", tol=tol).to(dev)
    per_round = EB.alternate(net, Adam(net.parameters(), lr=1e-3), batches, rounds, min(5, steps))
    return {m: {"step_ms": round(float(np.median(v)), 3), "step_ms_rounds": v} for m, v in per_round.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--qc-steps", type=int, default=20)
    ap.add_argument("--only", default="gat,step,qc")
    a = ap.parse_args()
    only = a.only.split(",")
    dev = torch.device("cuda:0")
    out = {"gat": {}, "step": None, "qc": None}
    n, graph = citeseer(dev)
    if "gat" in only:
        print("%-6s %-6s %-14s %-9s %10s %6s %6s" % ("width", "tol", "method", "mode", "ms/step", "nfe_f", "nfe_b"))
        for name, d, H in WIDTHS:
            for tol in TOLS:
                res = time_gat(dev, n, graph, d, H, tol, a.rounds, a.steps)
                for (m, adjoint), r in res.items():
                    mode = "adjoint" if adjoint else "backprop"
                    print("%-6s %-6g %-14s %-9s %10.3f %6d %6d" % ((name, tol, m, mode) + r), flush=True)
                    out["gat"]["%s/%g/%s/%s" % (name, tol, m, mode)] = {"ms_per_step": round(r[0], 3), "nfe_f": r[1], "nfe_b": r[2]}
                torch.cuda.empty_cache()
    if "step" in only:
        out["step"] = time_adjoint_step(dev, n, graph)
        print("adjoint step, Citeseer 1x16, ms per attempt:", out["step"], flush=True)
    if "qc" in only:
        out["qc"] = time_qc(dev, a.rounds, a.qc_steps)
        print("QC EdgeODE1_K_Sum h=96 bosh3 1e-3, ms per step:", {k: v["step_ms"] for k, v in out["qc"].items()}, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
