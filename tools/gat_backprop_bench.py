#!/usr/bin/env python3
"""Training-step time of the Citeseer GAT ODE model (the C3 configurations of tools/config_bench.py: Citeseer's edge list,
ODEGCN3 with one head at width 16 and with 8 heads x 8) under the three ways its block gets gradients, in one process with
the modes taking turns round by round: the adjoint solve (adjoint=True), backprop through the solve on the fused sweep
(adjoint=False; gat_ode.GatOdeField, csrc/gat_driver.hip) and backprop through the solve on the generic path
(GatOdeField.BACKPROP_FUSED = False: every interval re-run as torch ops under autograd).  fwd + bwd + Adam, under rk4 (step
0.25) and under dopri5 at each --tols value (rtol = atol).  Prints one JSON line: the median ms per step of every
configuration, method, mode and round.

  python tools/gat_backprop_bench.py [--steps 20] [--rounds 3] [--warmup 3] [--tols 1e-3,1e-5] [--methods rk4,dopri5]
                                     [--configs 1x16,8x8]
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
from graph_odenet_amd import gat_heads, gat_models, gat_ode, models  # noqa: E402
from graph_odenet_amd.optim import Adam  # noqa: E402

MODES = ("adjoint", "fused", "generic")
GOLD = os.path.join(ROOT, "tests", "golden")


def citeseer(dev):
    """Citeseer's edge list with the synthetic features and labels of tools/config_bench.py: c3_citeseer_gat."""
    g = dict(np.load(os.path.join(GOLD, "citeseer_gat_edges.npz")))
    n = int(g["n"])
    src, tgt = torch.from_numpy(g["src"].astype(np.int64)).to(dev), torch.from_numpy(g["tgt"].astype(np.int64)).to(dev)
    e = src.numel()
    Mtgt = torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(e, device=dev)]), torch.ones(e, device=dev), (n, e))
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(n, 3703, generator=gen) < 0.01).float()
    x = (x / x.sum(1, keepdim=True).clamp_min(1)).to(dev)
    y, idx = torch.randint(0, 6, (n,), generator=gen).to(dev), torch.arange(120, device=dev)
    return (x, src, tgt, Mtgt), y, idx


def alternate(net, opt, inputs, y, idx, steps, rounds, warmup):
    """{mode: per-round list of the median ms of a step}, the modes taking turns round by round."""
    blocks = [m for m in net.modules() if isinstance(m, models.ODEBlock)]

    def step():
        net.train()
        opt.zero_grad(set_to_none=True)
        F.nll_loss(net(*inputs)[idx], y[idx]).backward()
        opt.step()
    res, failed = {m: [] for m in MODES}, {}
    try:
        for _ in range(rounds):
            for mode in MODES:
                if mode in failed:
                    continue
                for b in blocks:
                    b.adjoint = mode == "adjoint"
                gat_ode.GatOdeField.BACKPROP_FUSED = mode != "generic"
                ts = []
                try:
                    for _ in range(warmup):
                        step()
                    for _ in range(steps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        step()
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                except RuntimeError as exc:
                    # only the solver's own giving up (solver.integrate_dopri5) leaves a mode out of the later rounds; any
                    # other error - a HIP error among them - ends the tool: nothing more is launched on a card that faulted
                    if "max_num_steps exceeded" not in str(exc):
                        raise
                    failed[mode] = "%s (after %d timed steps of round %d)" % (str(exc).splitlines()[0], len(ts), len(res[mode]))
                    continue
                res[mode].append(round(float(np.median(ts)), 3))
    finally:
        gat_ode.GatOdeField.BACKPROP_FUSED = True
    return res, failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps before the timed steps of every mode and round")
    ap.add_argument("--tols", default="1e-3,1e-5", help="rtol = atol of the dopri5 runs (1e-5: the reference's)")
    ap.add_argument("--methods", default="rk4,dopri5")
    ap.add_argument("--configs", default="1x16,8x8", help="heads x width per head")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    inputs, y, idx = citeseer(dev)
    out = {"metric": "Citeseer GAT ODEGCN3 fwd+bwd+Adam step, ms (median over the steps of a round), by gradient mode",
           "nodes": int(inputs[0].shape[0]), "edges": int(inputs[1].numel()), "steps_per_round": args.steps}
    runs = []
    for method in args.methods.split(","):
        if method == "rk4":
            runs.append(("rk4", dict(method="rk4", step_size=0.25)))
        else:
            runs += [("dopri5 tol %s" % t, dict(method=None, tol=float(t))) for t in args.tols.split(",")]
    for cfg in args.configs.split(","):
        heads, width = (int(v) for v in cfg.split("x"))
        zoo = gat_models if heads == 1 else gat_heads.zoo(heads)
        res = {}
        for name, kw in runs:
            torch.manual_seed(0)
            net = zoo.ODEGCN3(nfeat=inputs[0].shape[1], nhid=heads * width, nclass=6, dropout=0.5, **kw).to(dev)
            per_round, failed = alternate(net, Adam(net.parameters(), lr=0.01, weight_decay=5e-4), inputs, y, idx, args.steps,
                                          args.rounds, args.warmup)
            res[name] = dict({m: {"step_ms": round(float(np.median(v)), 3) if v else None, "step_ms_rounds": v}
                              for m, v in per_round.items()},
                             fused_below_generic_every_round=all(a < b for a, b in zip(per_round["fused"], per_round["generic"])),
                             **({"failed": failed} if failed else {}))
            print("%d x %d %s: %s" % (heads, width, name, json.dumps(res[name])), file=sys.stderr, flush=True)
        out["%d head(s) x %d" % (heads, width)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
