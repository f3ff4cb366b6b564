#!/usr/bin/env python3
"""The adaptive methods side by side: ms per training step (forward + adjoint backward + Adam) and nfe forward / backward of
dopri5, bosh3 and adaptive_heun at rtol = atol = 1e-3 and 1e-5 on

  cora      Cora, ODEGCN3 (GCN layers, hidden 16)
  pubmed    Pubmed topology, GCN-dense-paper ODEGCN3 (hidden 16; synthetic features)
  citeseer  Citeseer edge list, GAT ODEGCN3 with one head x 16 (synthetic features)

The methods take turns (one round = every method once, in order) and the figure is the median of 3 rounds; every model is
built once per (configuration, method, tolerance) from the same seed, so the weights - and with them the step sequences -
are those of a first training step plus the warm-up's updates.

Then the step close on its own: gode_rk_close_err_multi_f32 (2 launches) against gode_lincomb_f32 + gode_rk_errnorm_f32
(3 launches) on 5 terms at 2 708 x 16 and 2^20 x 128, through the Python wrappers both (so the small size is mostly the host
cost of two calls against one).

`python tools/adaptive_bench.py [--rounds 3] [--steps 10]` prints a table and one JSON object on the last line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
METHODS = ("dopri5", "bosh3", "adaptive_heun")
TOLS = (1e-3, 1e-5)


def _trainer(m, fwd, idx, y):
    from graph_odenet_amd.optim import Adam
    opt = Adam(m.parameters(), lr=0.01, weight_decay=5e-4)

    def step():
        m.train(); opt.zero_grad(); m.nfe = 0
        out = fwd()
        nf = m.nfe; m.nfe = 0
        F.nll_loss(out[idx], y[idx]).backward(); opt.step()
        return nf, m.nfe
    return step


def _T(a):
    return torch.from_numpy(np.asarray(a))


def cora(dev):
    from graph_odenet_amd import models
    g = dict(np.load(os.path.join(GOLD, "cora_graph.npz")))
    n = int(g["n"])
    adj = torch.sparse_coo_tensor(torch.stack([_T(g["rows"].astype(np.int64)), _T(g["cols"].astype(np.int64))]), _T(g["vals"]),
                                  (n, n)).to(dev)
    x = torch.zeros(n, int(g["n_feat"]))
    x[_T(g["feat_rows"].astype(np.int64)), _T(g["feat_cols"].astype(np.int64))] = _T(g["feat_vals"])
    x, y, idx = x.to(dev), _T(g["labels"].astype(np.int64)).to(dev), _T(g["idx_train"].astype(np.int64)).to(dev)

    def make(method, tol):
        torch.manual_seed(0)
        m = models.ODEGCN3(nfeat=x.shape[1], nhid=16, nclass=7, dropout=0.5, method=method, tol=tol).to(dev)
        return _trainer(m, lambda: m(x, adj), idx, y)
    return make


def pubmed(dev):
    from graph_odenet_amd import dense_paper
    g = dict(np.load(os.path.join(GOLD, "pubmed_graph_sym.npz")))
    n = int(g["n"])
    idx = torch.stack([_T(g["rows"].astype(np.int64)), _T(g["cols"].astype(np.int64))])
    adj = torch.sparse_coo_tensor(idx, _T(g["vals"]), (n, n)).to(dev).to_dense()
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(n, 500, generator=gen) < 0.1).float()
    x = (x / x.sum(1, keepdim=True).clamp_min(1)).to(dev)
    y, tr = torch.randint(0, 3, (n,), generator=gen).to(dev), torch.arange(60, device=dev)

    def make(method, tol):
        torch.manual_seed(0)
        m = dense_paper.ODEGCN3(nfeat=500, nhid=16, nclass=3, dropout=0.5, method=method, tol=tol).to(dev)
        return _trainer(m, lambda: m(x, adj), tr, y)
    return make


def citeseer(dev):
    from graph_odenet_amd import gat_models
    g = dict(np.load(os.path.join(GOLD, "citeseer_gat_edges.npz")))
    n = int(g["n"])
    src, tgt = _T(g["src"].astype(np.int64)).to(dev), _T(g["tgt"].astype(np.int64)).to(dev)
    e = src.numel()
    Mtgt = torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(e, device=dev)]), torch.ones(e, device=dev), (n, e))
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(n, 3703, generator=gen) < 0.01).float()
    x = (x / x.sum(1, keepdim=True).clamp_min(1)).to(dev)
    y, idx = torch.randint(0, 6, (n,), generator=gen).to(dev), torch.arange(120, device=dev)

    def make(method, tol):
        torch.manual_seed(0)
        m = gat_models.ODEGCN3(nfeat=3703, nhid=16, nclass=6, dropout=0.5, method=method, tol=tol).to(dev)
        return _trainer(m, lambda: m(x, src, tgt, Mtgt), idx, y)
    return make


CONFIGS = (("cora_odegcn3_h16", cora), ("pubmed_dense_paper_h16", pubmed), ("citeseer_gat_1x16", citeseer))


def time_methods(make, tol, rounds, steps, warm=3):
    """{method: (median ms per step over the rounds, nfe forward, nfe backward of the last step)}; methods alternate."""
    fns = {m: make(m, tol) for m in METHODS}
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ms = {m: [] for m in METHODS}
    nfe = {}
    for _ in range(rounds):
        for m in METHODS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                nfe[m] = fns[m]()
            torch.cuda.synchronize()
            ms[m].append(1e3 * (time.perf_counter() - t0) / steps)
    return {m: (sorted(ms[m])[len(ms[m]) // 2],) + tuple(nfe[m]) for m in METHODS}


def time_close(dev, shape, reps):
    """ms per step close: (fused 2 launches, separate 3 launches), 5 terms, CUDA events around `reps` calls each, 3 turns,
    median."""
    from graph_odenet_amd import ops
    n = shape[0] * shape[1]
    terms = [torch.randn(n, device=dev) for _ in range(5)]
    coef, ecoef = [1.0, 0.1, 0.2, 0.3, 0.0], [0.0, 0.01, -0.02, 0.015, -0.005]
    y1 = torch.empty(n, device=dev)
    sol = list(zip(coef, terms))
    sol_nz = [(c, t) for c, t in sol if c != 0.0]
    err_nz = [(c, t) for c, t in zip(ecoef, terms) if c != 0.0]
    out1, out2 = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)

    def fused():
        ops.rk_close_err_multi([y1], [sol], [ecoef], 1e-3, 1e-3, out=out1)

    def separate():
        ops.lincomb_(y1, sol_nz)
        ops.rk_error_sumsq(terms[0], y1, err_nz, 1e-3, 1e-3, out=out2)
    res = {"fused": [], "separate": []}
    for _ in range(3):
        for name, fn in (("fused", fused), ("separate", separate)):
            for _ in range(5):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            res[name].append(a.elapsed_time(b) / reps)
    return {k: sorted(v)[1] for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default=None, help="prefix of a configuration name")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"steps": {}, "close": {}}
    print("%-24s %-6s %-14s %10s %6s %6s" % ("configuration", "tol", "method", "ms/step", "nfe_f", "nfe_b"))
    for name, build in CONFIGS:
        if a.only and not name.startswith(a.only):
            continue
        make = build(dev)
        for tol in TOLS:
            res = time_methods(make, tol, a.rounds, a.steps)
            for m in METHODS:
                print("%-24s %-6g %-14s %10.3f %6d %6d" % ((name, tol, m) + res[m]), flush=True)
                out["steps"]["%s/%g/%s" % (name, tol, m)] = {"ms_per_step": round(res[m][0], 3), "nfe_f": res[m][1], "nfe_b": res[m][2]}
        torch.cuda.empty_cache()
    if not a.only:
        for shape, reps in (((2708, 16), 200), ((1 << 20, 128), 20)):
            r = time_close(dev, shape, reps)
            print("step close %8d x %-4d 5 terms: fused %.4f ms, lincomb + errnorm %.4f ms" % (shape + (r["fused"], r["separate"])), flush=True)
            out["close"]["%dx%d" % shape] = {k: round(v, 4) for k, v in r.items()}
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
