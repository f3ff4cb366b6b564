"""Long and short records of the benchmark's SpMM timed apart (d = 128, R-MAT 2^20 rows / 10 M edges, after tuned_graph).

The record list is sorted by length, longest first (graph.py), so a prefix and a suffix of `items` are the two phases of a
launch: records longer than SHORT (4) entries, which spend their time in gather rounds, and the rest, which spend it in
the dependent round trips before and after their one round (items, col / val, gathers, epilogue operands).  Each of

    long   items[:k], n_items = k, the graph's long_rows (the finishing launch runs and is inside the timing)
    short  items[k:], n_long = 0
    all    the whole list

is driven through gode_spmm_csr_f32 for A and A^T (rows a sub-list does not own stay unwritten), as the plain product and
with the epilogue of an adjoint stage (bias, relu, two cot terms, Y2, per-block column sums), under every value of the
run-time option spmm_pipe given with --pipe (0 = one tile per block, the kernel before the option existed; a launch
with a cotangent output runs that kernel under every setting).  HIP events,
2 warm-up and 10 timed launches, median.  Bytes of a part: gathered rows x 512 + stored rows x 512 x outputs (Y, and Y2
with the epilogue; a split record stores its slab row) + epilogue operand rows read x 512 + 8 per non-zero + 16 per record.

    python tools/spmm_phase_probe.py [--pipe 0,1] [--scale 20] [--edges 10000000] > profiles/spmm_phase_probe.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHORT = 4
D = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--pipe", default="0,1", help="values of the option spmm_pipe, one table each")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=10)
    args = ap.parse_args()
    from graph_odenet_amd import _lib, gcn_ode
    from graph_odenet_amd.synth import rmat_graph
    lib = _lib.load()
    assert torch.cuda.is_available(), "spmm_phase_probe.py needs a GPU"
    dev = torch.device("cuda", 0)
    g0 = rmat_graph(args.scale, args.edges, seed=0, device=dev)
    g0.transpose()
    g, order, _ = gcn_ode.tuned_graph(g0, D)
    print("graph: %d rows, %d non-zeros, renumbered %s" % (g.n_rows, g.nnz, order is not None))
    n = g.n_rows
    gen = torch.Generator(device=dev).manual_seed(7)
    X = torch.randn(n, D, generator=gen, device=dev)
    bias = torch.randn(D, generator=gen, device=dev)
    cot = [(0.5, torch.randn(n, D, generator=gen, device=dev)), (-1.25, torch.randn(n, D, generator=gen, device=dev))]
    Y = torch.zeros(n, D, device=dev)
    Y2 = torch.zeros(n, D, device=dev)

    def parts(gr):
        items = gr.items
        ln = (items[:, 2] - items[:, 1]).long()
        k = int((ln > SHORT).sum())
        assert bool((ln[:k] > SHORT).all()) and bool((ln[k:] <= SHORT).all())
        out = []
        for name, lo, hi, n_long in (("long", 0, k, gr.n_long), ("short", k, gr.n_items, 0), ("all", 0, gr.n_items, gr.n_long)):
            sub = items[lo:hi]
            nnz = int(ln[lo:hi].sum())
            slabs = int((sub[:, 3] >= 0).sum())                      # records of split rows: they store a slab row
            out.append((name, lo, hi - lo, n_long, nnz, slabs, gr.n_slots if n_long else 0))
        return k, out

    def launch(gr, lo, cnt, n_long, ep, colsum):
        if ep is not None:
            ep.Y2_colsum = colsum.data_ptr()
        rc = lib.gode_spmm_csr_f32(_lib.ptr(gr.rowptr), _lib.ptr(gr.col), _lib.ptr(gr.val),
                                   gr.items.data_ptr() + 16 * lo, cnt, _lib.ptr(gr.long_rows) if n_long else None, n_long,
                                   _lib.ptr(gr.partial(D)), _lib.ptr(X), D, _lib.ptr(Y), D, gr.n_rows, D,
                                   ctypes.byref(ep) if ep is not None else None, _lib.stream_ptr())
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

    old = lib.gode_get_option(b"spmm_pipe")
    try:
        for pipe in [int(t) for t in args.pipe.split(",")]:
            assert lib.gode_set_option(b"spmm_pipe", pipe) == 0 and lib.gode_get_option(b"spmm_pipe") == pipe
            print("\nspmm_pipe %d" % pipe)
            print("%-3s %-5s %-8s %9s %10s %9s %9s %9s %9s" % ("", "part", "epilogue", "records", "non-zeros", "MB", "ms", "min..max", "GB/s"))
            for gname, gr in (("A", g), ("A^T", g.transpose())):
                k, pl = parts(gr)
                for name, lo, cnt, n_long, nnz, slabs, slabs_read in pl:
                    for epi in ("plain", "adjoint"):
                        ep, colsum = None, None
                        outputs, operands = 1, 0
                        if epi == "adjoint":
                            ep = _lib.SpmmEpilogue()
                            ep.bias, ep.relu, ep.alpha = bias.data_ptr(), 1, 1.0
                            ep.cot = _lib.lincomb(cot)
                            ep.Y2 = Y2.data_ptr()
                            colsum = torch.empty(int(lib.gode_spmm_y2_colsum_rows(cnt, n_long, D)), D, device=dev)
                            assert colsum.numel() > 0
                            outputs, operands = 2, len(cot)
                        rows_out = cnt - slabs + n_long                           # rows that pass the epilogue
                        nbytes = (nnz * 4 * D + (slabs + slabs_read) * 4 * D + rows_out * 4 * D * (outputs + operands)
                                  + nnz * 8 + cnt * 16 + n_long * 16)
                        med, lo_ms, hi_ms = timed(lambda: launch(gr, lo, cnt, n_long, ep, colsum))
                        print("%-3s %-5s %-8s %9d %10d %9.1f %9.4f %4.3f..%4.3f %9.0f"
                              % (gname, name, epi, cnt, nnz, nbytes / 1e6, med, lo_ms, hi_ms, nbytes / med / 1e6), flush=True)
    finally:
        lib.gode_set_option(b"spmm_pipe", old)


if __name__ == "__main__":
    main()
