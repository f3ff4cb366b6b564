#!/usr/bin/env python3
"""Training-step time of the Citeseer GAT ODE model (Citeseer's edge list, ODEGCN3 with one head at width 16 and with
8 heads x 8) by the message activation of the ODE function's attention layer, in one process with the variants taking turns
round by round:

  relu fused     the reference's activation on the fused fields (gat_ode.py; the ActRelu kernels)
  elu fused      F.elu on the fused fields (gode_gat_act_t with outer_relu: message activation inside, the function's relu outside)
  tanh fused     torch.tanh likewise
  elu unfused    F.elu with the function's gode_fields hook giving None: every evaluation as autograd through the layer
                 (odeint.AutogradField) - what any activation but relu cost before the fused fields took one

fwd + bwd + Adam under rk4 (step 0.25) and under dopri5 at --tol (rtol = atol), the block trained through the adjoint solve
(adjoint=True) and through backprop through the solve (adjoint=False: the fused sweep of csrc/gat_driver.hip for the fused
variants, every interval re-run as torch ops under autograd for the unfused one).  Prints one JSON line: the median ms per
step of every configuration, method, gradient mode, variant and round.

  python tools/gat_ode_act_bench.py [--steps 15] [--rounds 3] [--warmup 3] [--tol 1e-3] [--methods rk4,dopri5]
                                    [--configs 1x16,8x8] [--variants "relu fused,elu fused,tanh fused,elu unfused"]
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
from graph_odenet_amd import gat_heads, gat_models, models  # noqa: E402
from graph_odenet_amd.optim import Adam  # noqa: E402

VARIANTS = {"relu fused": (None, True), "elu fused": (F.elu, True), "tanh fused": (torch.tanh, True), "elu unfused": (F.elu, False)}
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


def build(zoo, nfeat, nhid, kw, variant, adjoint, dev):
    """ODEGCN3 with the variant's activation on the ODE function's layer (relu: the layer as the zoo builds it)."""
    act, fused = VARIANTS[variant]
    torch.manual_seed(0)
    net = zoo.ODEGCN3(nfeat=nfeat, nhid=nhid, nclass=6, dropout=0.5, **kw).to(dev)
    for m in net.modules():
        if isinstance(m, models.ODEBlock):
            m.adjoint = adjoint
            if act is not None:
                m.odefunc.gc1.act = act
                for hd in getattr(m.odefunc.gc1, "heads", ()):
                    hd.act = act
            if not fused:
                m.odefunc.gode_fields = lambda y0: None              # the hook declines: odeint takes the autograd field
    return net, Adam(net.parameters(), lr=0.01, weight_decay=5e-4)


def alternate(nets, inputs, y, idx, steps, rounds, warmup):
    """{variant: per-round list of the median ms of a step}, the variants taking turns round by round."""
    def step(net, opt):
        net.train()
        opt.zero_grad(set_to_none=True)
        F.nll_loss(net(*inputs)[idx], y[idx]).backward()
        opt.step()
    res, failed = {v: [] for v in nets}, {}
    for _ in range(rounds):
        for v, (net, opt) in nets.items():
            if v in failed:
                continue
            ts = []
            try:
                for _ in range(warmup):
                    step(net, opt)
                for _ in range(steps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    step(net, opt)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
            except RuntimeError as exc:
                # only the solver's own giving up (solver.integrate_dopri5) leaves a variant out of the later rounds; any other
                # error - a HIP error among them - ends the tool: nothing more is launched on a card that faulted
                if "max_num_steps exceeded" not in str(exc):
                    raise
                failed[v] = "%s (after %d timed steps of round %d)" % (str(exc).splitlines()[0], len(ts), len(res[v]))
                continue
            res[v].append(round(float(np.median(ts)), 3))
    return res, failed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps before the timed steps of every variant and round")
    ap.add_argument("--tol", type=float, default=1e-3, help="rtol = atol of the dopri5 runs")
    ap.add_argument("--methods", default="rk4,dopri5")
    ap.add_argument("--configs", default="1x16,8x8", help="heads x width per head")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    inputs, y, idx = citeseer(dev)
    variants = [v.strip() for v in args.variants.split(",")]
    out = {"metric": "Citeseer GAT ODEGCN3 fwd+bwd+Adam step, ms (median over the steps of a round), by message activation",
           "nodes": int(inputs[0].shape[0]), "edges": int(inputs[1].numel()), "steps_per_round": args.steps}
    runs = []
    for method in args.methods.split(","):
        runs.append(("rk4 step 1/4", dict(method="rk4", step_size=0.25)) if method == "rk4"
                    else ("dopri5 tol %g" % args.tol, dict(method=None, tol=args.tol)))
    for cfg in args.configs.split(","):
        heads, width = (int(v) for v in cfg.split("x"))
        zoo = gat_models if heads == 1 else gat_heads.zoo(heads)
        res = {}
        for name, kw in runs:
            for adjoint in (True, False):
                mode = "adjoint" if adjoint else "backprop"
                nets = {v: build(zoo, inputs[0].shape[1], heads * width, kw, v, adjoint, dev) for v in variants}
                per_round, failed = alternate(nets, inputs, y, idx, args.steps, args.rounds, args.warmup)
                res["%s, %s" % (name, mode)] = dict({v: {"step_ms": round(float(np.median(r)), 3) if r else None, "step_ms_rounds": r}
                                                     for v, r in per_round.items()}, **({"failed": failed} if failed else {}))
                print("%d x %d %s %s: %s" % (heads, width, name, mode, json.dumps(res["%s, %s" % (name, mode)])), file=sys.stderr,
                      flush=True)
                del nets
        out["%d head(s) x %d" % (heads, width)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
