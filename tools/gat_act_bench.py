#!/usr/bin/env python3
"""GAT layer forward + backward with message activations other than relu: the aggregation kernels' activation argument
(relu, elu, tanh on the kernel path) against the general path (elu passed as a lambda, which message_activation does not
recognise: messages formed per edge with PyTorch ops).  Inputs as tools/gat_bench.py / tools/gat_scale.py build them:
  * Citeseer's edge list, 64 -> 64 features, 1 and 8 heads;
  * R-MAT scale 20 / 10 M edges, 128 -> 128 features, one head, peak memory too.
Time: ms per forward + backward, median of 3 rounds; the variants alternate inside every round.  Development aid.
usage: gat_act_bench.py [citeseer] [rmat]"""
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_odenet_amd import gat_layers  # noqa: E402
from graph_odenet_amd.gat_heads import MultiHeadGraphConvolution  # noqa: E402
from graph_odenet_amd.gat_layers import GraphConvolution, message_activation  # noqa: E402
from graph_odenet_amd.synth import rmat_graph  # noqa: E402

dev = torch.device("cuda:0")
VARIANTS = (("relu kernels", F.relu), ("elu kernels", F.elu), ("tanh kernels", torch.tanh), ("elu general", lambda v: F.elu(v)))
ROUNDS = 3


def citeseer():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "citeseer_gat_edges.npz")))
    n = int(g["n"])
    return n, torch.from_numpy(g["src"].astype(np.int64)).to(dev), torch.from_numpy(g["tgt"].astype(np.int64)).to(dev)


def rmat():
    g = rmat_graph(20, 10_000_000, seed=0, device=dev)
    n = g.n_rows
    rp = g.rowptr.to(torch.int64)
    tgt = torch.repeat_interleave(torch.arange(n, device=dev), rp[1:] - rp[:-1])
    return n, g.col.to(torch.int64), tgt


def bench(title, n, src, tgt, width, heads, iters, memory=False):
    E = src.numel()
    Mtgt = torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(E, device=dev)]), torch.ones(E, device=dev), (n, E))
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(n, width, generator=gen).to(dev).requires_grad_(True)
    gout = torch.randn(n, width, generator=gen).to(dev)
    general_calls = []
    general = gat_layers._gat_forward_general

    def counting(*a, **k):
        general_calls.append(1)
        return general(*a, **k)

    gat_layers._gat_forward_general = counting
    layers, times, peak = {}, {}, {}
    for name, act in VARIANTS:
        torch.manual_seed(0)
        layer = GraphConvolution(width, width, act=act) if heads == 1 else MultiHeadGraphConvolution(width, width, heads=heads, act=act)
        layers[name], times[name] = layer.to(dev), []

    def step(layer):
        x.grad = None
        layer.zero_grad(set_to_none=True)
        layer(x, src, tgt, Mtgt).backward(gout)

    for name, layer in layers.items():                               # warm-up; which path ran; peak memory of one step
        del general_calls[:]
        step(layer)
        torch.cuda.synchronize()
        want = 0 if message_activation(layer.act) is not None else heads
        assert len(general_calls) == want, (name, len(general_calls), want)
        if memory:
            x.grad = None
            layer.zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(layer)
            torch.cuda.synchronize()
            peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    for _ in range(ROUNDS):
        for name, layer in layers.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(iters):
                step(layer)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / iters * 1e3)
    gat_layers._gat_forward_general = general
    for name in layers:
        t = times[name]
        mem = "  peak memory of a step above the inputs %.2f GB" % peak[name] if memory else ""
        print("%s  N=%d E=%d  %-13s %8.3f ms fwd+bwd (median of %d rounds of %d; min %.3f max %.3f)%s"
              % (title, n, E, name, statistics.median(t), ROUNDS, iters, min(t), max(t), mem), flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["citeseer", "rmat"]
    if "citeseer" in which:
        n, src, tgt = citeseer()
        for heads in (1, 8):
            bench("citeseer o=64 heads=%d" % heads, n, src, tgt, 64, heads, iters=50)
    if "rmat" in which:
        n, src, tgt = rmat()
        bench("rmat20 o=128 heads=1", n, src, tgt, 128, 1, iters=10, memory=True)
