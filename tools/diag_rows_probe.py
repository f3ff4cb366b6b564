"""What the plain SpMM of the benchmark spends on diagonal-only rows (d = 128, R-MAT 2^20 rows / 10 M edges, after
tuned_graph): the premise of running the ODE block's plain products on the core record list (CSRGraph.diag_rows).

For A and A^T the plain product is driven through gode_spmm_csr_f32 once on the whole record list and once on the core
list (the records of the rows whose only entry is their own non-zero diagonal taken out; those rows stay unwritten).
HIP events, 2 warm-up and 10 timed launches, median, as tools/spmm_phase_probe.py does.  The two lists are timed
alternately (full, core, full, core, ...) in --rounds rounds, so that a drift of the clock shows as a spread among the
rounds and not as a difference between the lists.

Then the two launches of an adjoint stage that the option diag_rows changes, timed apart: Sp(g) with the cotangent
epilogue (which stores the isolated rows' share of A^T dZ itself) and SpT(g) on A^T's list without those rows - with no
row taken out, with n / 8 of them (the share at which gcn_ode.tuned_graph starts to hand the list over) and with all.

Last, the product of the forward solve's last stage (section "last"): relu, bias, pre = {1.0, P} read and overwritten in
place, alpha = h b_3 - on A's whole list against A's core list, alternating as above.  That is the premise of taking the
diagonal-only rows out of that launch as well (option diag_last).

    python tools/diag_rows_probe.py [--scale 20] [--edges 10000000] > profiles/diag_rows_probe.txt
    python tools/diag_rows_probe.py --sections last > profiles/diag_last_probe.txt
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


def last_stage(args, lib, _lib, g, S, timed, ode_steps=16):
    """Sp(3) of a forward rk4 step: y_new = P + h b_3 relu(A S + b), P and y_new in one array."""
    n = g.n_rows
    dr = g.diag_rows()
    gen = torch.Generator(device=S.device).manual_seed(8)
    bias = torch.randn(D, generator=gen, device=S.device)
    P = torch.randn(n, D, generator=gen, device=S.device)
    alpha = (1.0 / ode_steps) * 0.125                        # h b_3 of the 3/8 rule

    def launch(items, cnt):
        ep = _lib.SpmmEpilogue()
        ep.bias, ep.relu, ep.alpha, ep.n_items_full = bias.data_ptr(), 1, alpha, g.n_items
        ep.pre = _lib.lincomb([(1.0, P)])
        _lib.check(lib.gode_spmm_csr_f32(_lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val), _lib.ptr(items), cnt,
                                         _lib.ptr(g.long_rows), g.n_long, _lib.ptr(g.partial(D)), _lib.ptr(S), D, _lib.ptr(P), D,
                                         n, D, ctypes.byref(ep), _lib.stream_ptr()), "gode_spmm_csr_f32")

    print("last stage of a forward rk4 step: relu, bias, pre = {1.0, P} in place, alpha = %.6f; A flags %d of %d rows (%.2f %%)"
          % (alpha, dr.n_flagged, n, 100.0 * dr.n_flagged / n))
    print("%-5s %-5s %9s %9s %13s" % ("round", "list", "records", "ms", "min..max"))
    med = {"full": [], "core": []}
    for r in range(args.rounds):
        for lname, items, cnt in (("full", g.items, g.n_items), ("core", dr.items, dr.n_items)):
            m, lo, hi = timed(lambda: launch(items, cnt))
            med[lname].append(m)
            print("%-5d %-5s %9d %9.4f %5.3f..%5.3f" % (r, lname, cnt, m, lo, hi), flush=True)
    full, core = statistics.median(med["full"]), statistics.median(med["core"])
    print("last stage: full %.4f ms, core %.4f ms, difference %.4f ms per launch (spread among rounds: full %.4f, core %.4f); "
          "the rule: build the dense form only if the difference is at least 0.05 ms\n"
          % (full, core, full - core, max(med["full"]) - min(med["full"]), max(med["core"]) - min(med["core"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sections", default="plain,adjoint,last", help="which of the three parts to run")
    args = ap.parse_args()
    sections = set(args.sections.split(","))
    assert sections and sections <= {"plain", "adjoint", "last"}, args.sections
    from graph_odenet_amd import _lib, gcn_ode
    from graph_odenet_amd.synth import rmat_graph
    lib = _lib.load()
    assert torch.cuda.is_available(), "diag_rows_probe.py needs a GPU"
    dev = torch.device("cuda", 0)
    g0 = rmat_graph(args.scale, args.edges, seed=0, device=dev)
    g0.transpose()
    g, order, _ = gcn_ode.tuned_graph(g0, D)
    n = g.n_rows
    print("graph: %d rows, %d non-zeros, renumbered %s" % (n, g.nnz, order is not None))
    gen = torch.Generator(device=dev).manual_seed(7)
    X = torch.randn(n, D, generator=gen, device=dev)
    Y = torch.zeros(n, D, device=dev)

    def launch(gr, items, cnt):
        rc = lib.gode_spmm_csr_f32(_lib.ptr(gr.rowptr), _lib.ptr(gr.col), _lib.ptr(gr.val), _lib.ptr(items), cnt,
                                   _lib.ptr(gr.long_rows), gr.n_long, _lib.ptr(gr.partial(D)), _lib.ptr(X), D,
                                   _lib.ptr(Y), D, gr.n_rows, D, None, _lib.stream_ptr())
        _lib.check(rc, "gode_spmm_csr_f32")

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

    both = (g.diag_rows().diag != 0) & (g.transpose().diag_rows().diag != 0)
    print("diagonal-only in A and in A^T: %d rows (%.2f %%)" % (int(both.sum()), 100.0 * int(both.sum()) / n))
    if "plain" in sections:
        print("\n%-3s %-5s %-5s %9s %9s %9s %13s" % ("", "round", "list", "records", "MB", "ms", "min..max"))
    for gname, gr in (("A", g), ("A^T", g.transpose())) if "plain" in sections else ():
        dr = gr.diag_rows()
        lists = (("full", gr.items, gr.n_items), ("core", dr.items, dr.n_items))
        med = {"full": [], "core": []}
        for r in range(args.rounds):
            for lname, items, cnt in lists:
                flagged = gr.n_items - cnt
                # the algorithmic bytes of the matrix less a row read, a row written, the entry and the record
                nbytes = gr.algorithmic_bytes(D) + gr.n_items * 16 - flagged * (8 * D + 8 + 16)
                m, lo, hi = timed(lambda: launch(gr, items, cnt))
                med[lname].append(m)
                print("%-3s %-5d %-5s %9d %9.1f %9.4f %5.3f..%5.3f" % (gname, r, lname, cnt, nbytes / 1e6, m, lo, hi), flush=True)
        full, core = statistics.median(med["full"]), statistics.median(med["core"])
        print("%-3s flagged %d of %d rows (%.2f %%): full %.4f ms, core %.4f ms, difference %.4f ms per launch "
              "(spread among rounds: full %.4f, core %.4f)\n"
              % (gname, dr.n_flagged, n, 100.0 * dr.n_flagged / n, full, core, full - core,
                 max(med["full"]) - min(med["full"]), max(med["core"]) - min(med["core"])), flush=True)

    if "last" in sections:
        last_stage(args, lib, _lib, g, X, timed)
    if "adjoint" not in sections:
        return

    # ---- the pair of an adjoint stage: Sp(g) with the cotangent epilogue (bias, relu, two terms, dZ, per-block column
    # sums), then SpT(g) = A^T dZ.  "full": as before the option; "isolated": Sp(g) stores a_ii dZ[i] of every isolated row
    # into dS, SpT(g) on A^T's list without them; "eighth": the same with only the first n / 8 isolated rows taken out -
    # the share at which gcn_ode.tuned_graph starts to hand the list over (its gate, measured on this graph).
    from graph_odenet_amd.graph import DiagRows
    gt = g.transpose()
    iso = gt.isolated_rows()
    flagged = iso.diag != 0
    eighth = DiagRows(gt, among=(flagged & (torch.cumsum(flagged.to(torch.int64), 0) <= n // 8)).float())
    bias = torch.randn(D, generator=gen, device=dev)
    cot = [(0.5, torch.randn(n, D, generator=gen, device=dev)), (-1.25, torch.randn(n, D, generator=gen, device=dev))]
    dZ, dS = torch.zeros(n, D, device=dev), torch.zeros(n, D, device=dev)
    colsum = torch.empty(int(lib.gode_spmm_y2_colsum_rows(g.n_items, g.n_long, D)), D, device=dev)

    def sp(core):
        ep = _lib.SpmmEpilogue()
        ep.bias, ep.relu, ep.alpha = bias.data_ptr(), 1, 1.0
        ep.cot = _lib.lincomb(cot)
        ep.Y2, ep.Y2_colsum = dZ.data_ptr(), colsum.data_ptr()
        if core is not None:
            ep.Y2_scale, ep.Y2_scaled = core.diag.data_ptr(), dS.data_ptr()
        _lib.check(lib.gode_spmm_csr_f32(_lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val), _lib.ptr(g.items), g.n_items,
                                         _lib.ptr(g.long_rows), g.n_long, _lib.ptr(g.partial(D)), _lib.ptr(X), D, _lib.ptr(Y), D,
                                         n, D, ctypes.byref(ep), _lib.stream_ptr()), "gode_spmm_csr_f32")

    def spt(core):
        pt = _lib.SpmmEpilogue()
        pt.alpha, pt.n_items_full = 1.0, gt.n_items
        items, cnt = (gt.items, gt.n_items) if core is None else (core.items, core.n_items)
        _lib.check(lib.gode_spmm_csr_f32(_lib.ptr(gt.rowptr), _lib.ptr(gt.col), _lib.ptr(gt.val), _lib.ptr(items), cnt,
                                         _lib.ptr(gt.long_rows), gt.n_long, _lib.ptr(gt.partial(D)), _lib.ptr(dZ), D,
                                         _lib.ptr(dS), D, n, D, ctypes.byref(pt), _lib.stream_ptr()), "gode_spmm_csr_f32")

    print("adjoint stage pair: Sp(g) with the cotangent epilogue, SpT(g); isolated rows %d (%.2f %%), eighth %d"
          % (iso.n_flagged, 100.0 * iso.n_flagged / n, eighth.n_flagged))
    print("%-5s %-9s %9s %9s %9s" % ("round", "rows out", "Sp ms", "SpT ms", "pair ms"))
    res = {}
    for r in range(args.rounds):
        for name, core in (("none", None), ("eighth", eighth), ("isolated", iso)):
            a = timed(lambda: sp(core))[0]
            b = timed(lambda: spt(core))[0]
            res.setdefault(name, []).append((a, b))
            print("%-5d %-9s %9.4f %9.4f %9.4f" % (r, name, a, b, a + b), flush=True)
    med = {k: (statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)) for k, v in res.items()}
    for name in ("eighth", "isolated"):
        print("%-8s Sp %+.4f ms, SpT %+.4f ms, pair %+.4f ms against the full lists"
              % (name, med[name][0] - med["none"][0], med[name][1] - med["none"][1],
                 sum(med[name]) - sum(med["none"])), flush=True)


if __name__ == "__main__":
    main()
