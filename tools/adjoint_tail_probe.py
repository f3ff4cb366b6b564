"""The premise of option adjoint_tail, measured before any kernel: what Sp(g), the SpMM of the adjoint solve's forward
recompute with the cotangent epilogue, spends on the isolated tail rows [n - n_tail, n) of the benchmark graph (R-MAT 2^20
rows / 10 M edges after tuned_graph, d = 128).

Sp(g) is driven through gode_spmm_csr_f32 in the four stage forms the driver issues on the one-pass branch (bias, relu, dZ,
per-block column sums, Y2_scale = A^T's isolated diagonal, Y2_scaled = dS): 1, 2 and 3 cotangent terms, and stage 3 with
pre = {1.0, P} read and overwritten in place, alpha = h b_3, four terms and the third output.  Each form once on A's whole
record list (today's launch) and once on the list without the records of the tail rows (n_items_full = the whole count, so
the same kernels run).  HIP events, 2 warm-up and 10 timed launches, median; the two lists alternate (full, core, full,
core, ...) over --rounds rounds, as tools/diag_rows_probe.py does.

What a dense launch over the tail rows would pay for taking that work over is priced from bytes: per tail row and stage the
cotangent terms read ((s + 1) x 512 B) and two rows stored (1 024 B; at stage 3 a third, the closing combination of the
cotangent) less the S row (and at stage 3 the P row) that nobody stores any more (512 B each) - at the streaming rate of
the adjoint's dense forward launches, measured here as bench.py's roofline_dense prices them: arrays moved over duration, on
the forms that stream (3, 5 and 7 arrays at n rows).

The rule: go on only if the saving per launch exceeds that price by at least 0.05 ms on average over the four forms.

    python tools/adjoint_tail_probe.py [--scale 20] [--edges 10000000] > profiles/adjoint_tail_probe.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 128
BAR_MS = 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ode-steps", type=int, default=16)
    args = ap.parse_args()
    from graph_odenet_amd import _lib, gcn_ode
    from graph_odenet_amd.synth import rmat_graph
    lib = _lib.load()
    assert torch.cuda.is_available(), "adjoint_tail_probe.py needs a GPU"
    dev = torch.device("cuda", 0)
    g0 = rmat_graph(args.scale, args.edges, seed=0, device=dev)
    g0.transpose()
    g, order, _ = gcn_ode.tuned_graph(g0, D)
    n = g.n_rows
    n_tail = g.__dict__.get("_n_tail", 0)
    assert n_tail > 0, "no isolated tail on this graph"
    n_core = n - n_tail
    iso = g.transpose().isolated_rows()
    keep = g.items[:, 0].to(torch.int64) < n_core
    core_items = g.items[keep].contiguous()
    n_core_items = int(core_items.shape[0])
    assert n_core_items == g.n_items - n_tail                  # a tail row is one record
    print("graph: %d rows, %d non-zeros, renumbered %s; isolated %d, n_tail %d (%.2f %%), records %d -> %d"
          % (n, g.nnz, order is not None, iso.n_flagged, n_tail, 100.0 * n_tail / n, g.n_items, n_core_items))

    gen = torch.Generator(device=dev).manual_seed(7)
    S = torch.randn(n, D, generator=gen, device=dev)
    bias = torch.randn(D, generator=gen, device=dev)
    terms = [torch.randn(n, D, generator=gen, device=dev) for _ in range(4)]
    K, P = torch.zeros(n, D, device=dev), torch.randn(n, D, generator=gen, device=dev)
    dZ, dS, cot_out = (torch.zeros(n, D, device=dev) for _ in range(3))
    colsum = torch.empty(int(lib.gode_spmm_y2_colsum_rows(g.n_items, g.n_long, D)), D, device=dev)
    h = -1.0 / args.ode_steps                                  # the adjoint runs backwards
    xc = [[1.0], [1.0, h / 3], [1.0, -h / 3, h], [1.0, h, -h, h]]
    close = [1.0, h / 8, 3 * h / 8, 3 * h / 8]
    alpha = h / 8

    def sp(stage, items, cnt):
        ep = _lib.SpmmEpilogue()
        ep.bias, ep.relu, ep.alpha, ep.n_items_full = bias.data_ptr(), 1, 1.0, g.n_items
        ep.cot = _lib.lincomb([(-c, t) for c, t in zip(xc[stage], terms)])
        ep.Y2, ep.Y2_colsum = dZ.data_ptr(), colsum.data_ptr()
        ep.Y2_scale, ep.Y2_scaled = iso.diag.data_ptr(), dS.data_ptr()
        out = K
        if stage == 3:
            ep.pre, ep.alpha, out = _lib.lincomb([(1.0, P)]), alpha, P
            ep.cot_out = cot_out.data_ptr()
            for j in range(4):
                ep.cot_out_coef[j] = close[j]
        _lib.check(lib.gode_spmm_csr_f32(_lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val), _lib.ptr(items), cnt,
                                         _lib.ptr(g.long_rows), g.n_long, _lib.ptr(g.partial(D)), _lib.ptr(S), D, _lib.ptr(out), D,
                                         n, D, ctypes.byref(ep), _lib.stream_ptr()), "gode_spmm_csr_f32")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    # the streaming rate of the adjoint's dense forward launches, as bench.py's roofline_dense prices them (arrays moved over
    # the launch's duration): the forms that stream - two terms (3 arrays), three terms with x_out (5), four terms with x_out
    # and the closing combination (7).  The one-term form (2 arrays) is bound by its matrix phase, not by memory, and is listed
    # for that reason only.
    W = torch.randn(D + 1, D, generator=gen, device=dev) / D ** 0.5
    gam, bet = (torch.rand(D, generator=gen, device=dev) for _ in range(2))
    aux = (ctypes.c_float * 8)(*close, 0, 0, 0, 0)

    def gf(nt, xout, last):
        lc = _lib.lincomb(list(zip(xc[nt - 1], terms)))
        if last:
            rc = lib.gode_gn_time_gemm_xout_aux_f32(ctypes.byref(lc), n, D, 32, 1e-5, _lib.ptr(gam), _lib.ptr(bet), _lib.ptr(W), D, 1,
                                                    0.3, _lib.ptr(dZ), _lib.ptr(dS), aux, _lib.ptr(cot_out), _lib.stream_ptr())
        else:
            rc = lib.gode_gn_time_gemm_xout_f32(ctypes.byref(lc), n, D, 32, 1e-5, _lib.ptr(gam), _lib.ptr(bet), _lib.ptr(W), D, 1,
                                                0.3, _lib.ptr(dZ), _lib.ptr(dS) if xout else None, _lib.stream_ptr())
        _lib.check(rc, "gode_gn_time_gemm_xout_f32")
    rates = {}
    for r in range(args.rounds):
        for nt, xout, last, arrays in ((1, False, False, 2), (2, False, False, 3), (3, True, False, 5), (4, True, True, 7)):
            m = timed(lambda: gf(nt, xout, last))[0]
            rates.setdefault(arrays, []).append(arrays * n * D * 4 / (m * 1e-3) / 1e12)
    for arrays, v in rates.items():
        print("dense forward launch, %d arrays of %d rows: %s TB/s, median %.3f TB/s"
              % (arrays, n, " ".join("%.3f" % x for x in v), statistics.median(v)))
    rate = statistics.median([statistics.median(v) for arrays, v in rates.items() if arrays > 2])
    print("streaming rate taken (median of the three streaming forms): %.3f TB/s" % rate)

    print("\n%-6s %-5s %-5s %9s %9s %13s" % ("stage", "round", "list", "records", "ms", "min..max"))
    saving, price = [], []
    for stage in range(4):
        med = {"full": [], "core": []}
        for r in range(args.rounds):
            for lname, items, cnt in (("full", g.items, g.n_items), ("core", core_items, n_core_items)):
                m, lo, hi = timed(lambda: sp(stage, items, cnt))
                med[lname].append(m)
                print("%-6d %-5d %-5s %9d %9.4f %5.3f..%5.3f" % (stage, r, lname, cnt, m, lo, hi), flush=True)
        full, core = statistics.median(med["full"]), statistics.median(med["core"])
        row = 4 * D
        moved = n_tail * ((stage + 1) * row + (3 if stage == 3 else 2) * row - (2 if stage == 3 else 1) * row)
        pay = moved / (rate * 1e12) * 1e3
        saving.append(full - core)
        price.append(pay)
        print("stage %d (%d terms%s): full %.4f ms, without the tail %.4f ms, saving %.4f ms per launch (spread among rounds: "
              "full %.4f, core %.4f); the tail launch would pay %.1f MB = %.4f ms; net %.4f ms\n"
              % (stage, stage + 1, ", pre = {1, P}, third output" if stage == 3 else "", full, core, full - core,
                 max(med["full"]) - min(med["full"]), max(med["core"]) - min(med["core"]), moved / 1e6, pay, full - core - pay),
              flush=True)
    net = [s - p for s, p in zip(saving, price)]
    mean = sum(net) / 4
    print("net saving per launch, stages 0..3: %s ms; mean %.4f ms; the bar is %.2f ms: %s"
          % (" / ".join("%.4f" % x for x in net), mean, BAR_MS, "GO ON" if mean >= BAR_MS else "STOP"))
    print("per training step (64 launches): %.2f ms" % (16 * sum(net)))


if __name__ == "__main__":
    main()
