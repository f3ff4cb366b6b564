"""The premise of option local_tail, measured: the four dense launches of a forward rk4 step (gn_gemm_fwd_pc_kernel DIAG with
1, 2, 3 terms; AUX + DIAG with 4) on all n rows of the benchmark graph against its first n_core = n - n_tail rows, and the tail
launch (the whole 16-step forward solve of the n_tail isolated rows) alone, at several grids.

R-MAT 2^20 / 10 M edges after tuned_graph (hubs first), d = 128, GroupNorm(32).  HIP events around each launch; the two row
counts alternate in one process, --rounds rounds, the first one dropped (tools/dev/pc_ab.py's way).

    python tools/local_tail_probe.py [--scale 20] [--edges 10000000] [--rounds 6]
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    from graph_odenet_amd import _lib
    from graph_odenet_amd.gcn_ode import _graph_struct, tuned_graph
    from graph_odenet_amd.synth import rmat_graph
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    d = 128
    g0 = rmat_graph(args.scale, args.edges, seed=0, device=dev)
    g = tuned_graph(g0, d)[0]
    info = g0.__dict__["_tuned_info"][(d, "auto")]
    print("graph:", info)
    n, n_tail = g.n_rows, info["n_tail"]
    n_core = n - n_tail
    assert n_tail > 0, "no isolated tail on this graph"
    tail_diag = g.diag_rows().diag[n_core:]
    print("n %d  n_core %d (mod 32: %d)  n_tail %d  isolated %d  every a_ii of the tail == 1.0: %s"
          % (n, n_core, n_core % 32, n_tail, info["isolated_rows"], bool((tail_diag == 1.0).all())))
    gen = torch.Generator(device=dev).manual_seed(3)
    arr = [torch.randn(n, d, generator=gen, device=dev) for _ in range(4)]
    S, K = torch.empty(n, d, device=dev), torch.empty(n, d, device=dev)
    W = torch.randn(d + 1, d, generator=gen, device=dev) / d ** 0.5
    b, gam, bet = (torch.rand(d, generator=gen, device=dev) for _ in range(3))
    a_diag, skip = g.diag_rows().diag, g.transpose().isolated_rows().diag
    h = 1.0 / 16
    xc = [[1.0], [1.0, h / 3], [1.0, -h / 3, h], [1.0, h, -h, h]]
    ac = (ctypes.c_float * 8)(1.0, h / 8, 3 * h / 8, 3 * h / 8, 0, 0, 0, 0)
    taken = ctypes.c_int32(0)
    st = _lib.stream_ptr()

    def dense(s, rows):
        lc = _lib.lincomb(list(zip(xc[s], arr)))
        if s < 3:
            rc = lib.gode_gn_time_gemm_diag_f32(ctypes.byref(lc), rows, d, 32, 1e-5, _lib.ptr(gam), _lib.ptr(bet), _lib.ptr(W), d, 1,
                                                0.3, _lib.ptr(S), _lib.ptr(a_diag), _lib.ptr(skip), _lib.ptr(b), _lib.ptr(K),
                                                ctypes.byref(taken), st)
        else:
            rc = lib.gode_gn_time_gemm_diag_aux_f32(ctypes.byref(lc), rows, d, 32, 1e-5, _lib.ptr(gam), _lib.ptr(bet), _lib.ptr(W), d,
                                                    1, 0.3, _lib.ptr(S), ac, _lib.ptr(K), h / 8, _lib.ptr(a_diag), _lib.ptr(skip),
                                                    _lib.ptr(b), ctypes.byref(taken), st)
        assert rc == 0 and taken.value == 1

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    us = {(s, rows): [] for s in range(4) for rows in (n, n_core)}
    for r in range(args.rounds):
        for s in range(4):
            for rows in (n, n_core):
                t = timed(lambda: dense(s, rows))
                if r > 0:
                    us[(s, rows)].append(t)
    tot = {n: 0.0, n_core: 0.0}
    print("# dense launch (terms)      n rows [us]   n_core rows [us]   saved [us]")
    for s in range(4):
        a, c = (sum(us[(s, rows)]) / len(us[(s, rows)]) for rows in (n, n_core))
        tot[n] += a
        tot[n_core] += c
        print("%s %d terms        %10.1f   %14.1f   %10.1f" % ("AUX+DIAG" if s == 3 else "DIAG    ", s + 1, a, c, a - c))
    print("per rk4 step                %10.1f   %14.1f   %10.1f   (bar: 300 us saved)" % (tot[n], tot[n_core], tot[n] - tot[n_core]))

    # the tail launch alone: a whole 16-step forward solve of the tail rows through the driver's own door
    fs = _lib.GcnOdeFunc()
    fs.A, fs.AT = _graph_struct(g, d), _graph_struct(g.transpose(), d)
    fs.n, fs.d, fs.groups, fs.eps = n, d, 32, 1e-5
    fs.W, fs.b, fs.gamma, fs.beta = W.data_ptr(), b.data_ptr(), gam.data_ptr(), bet.data_ptr()
    core = g.__dict__["_at_core"]
    a = g.__dict__["_a_core"]
    fs.at_core_items, fs.at_n_core, fs.at_diag = core.items.data_ptr(), core.n_items, core.diag.data_ptr()
    fs.a_core_items, fs.a_n_core, fs.a_diag = a.items.data_ptr(), a.n_items, a.diag.data_ptr()
    fs.n_tail = n_tail
    ws = _lib.Rk4Workspace()
    ws.S = S.data_ptr()
    ky = [K] + [torch.empty(n, d, device=dev) for _ in range(3)]
    for i in range(4):
        ws.ky[i] = ky[i].data_ptr()
    res = ctypes.c_void_p()
    y = arr[0]
    prof = lib.gode_prof_create(1024)
    print("# tail launch (16 steps, %d rows) alone, by grid; and the forward solve's launches beside it" % n_tail)
    for blocks in (512, 256, 128, 64):
        for overlap in (1, 0):
            assert lib.gode_set_option(b"local_tail_blocks", blocks) == 0 and lib.gode_set_option(b"overlap", overlap) == 0
            rows = []
            for r in range(3):
                lib.gode_prof_reset(prof)
                lib.gode_prof_enable(prof)
                t = timed(lambda: lib.gode_gcn_ode_rk4_forward(ctypes.byref(fs), _lib.ptr(y), ctypes.byref(res), ctypes.byref(ws),
                                                               0.0, 1.0, 16, st))
                torch.cuda.synchronize()
                lib.gode_prof_enable(None)
                cnt = lib.gode_prof_count(prof)
                ms, rr, kk = (ctypes.c_float * cnt)(), (ctypes.c_int64 * cnt)(), (ctypes.c_int32 * cnt)()
                lib.gode_prof_read(prof, ms, None, rr, None, cnt)
                lib.gode_prof_kinds(prof, kk, cnt)
                tail = sum(ms[i] for i in range(cnt) if (kk[i] & 0xff) == 12)
                sp = [ms[i] for i in range(cnt) if kk[i] == 0]
                gf = sum(ms[i] for i in range(cnt) if (kk[i] & 0xff) == 1)
                rows.append((t / 1e3, tail, sum(sp), gf))
            t, tail, sp, gf = rows[-1]
            print("blocks %4d overlap %d: forward solve %8.2f ms   tail launch %6.2f ms   64 SpMM %7.2f ms   64 Gf %7.2f ms"
                  % (blocks, overlap, t, tail, sp, gf))
    for local in (1, 0):
        lib.gode_set_option(b"local_tail", local)
        lib.gode_set_option(b"local_tail_blocks", 0)
        lib.gode_set_option(b"overlap", 1)
        ts = [timed(lambda: lib.gode_gcn_ode_rk4_forward(ctypes.byref(fs), _lib.ptr(y), ctypes.byref(res), ctypes.byref(ws), 0.0, 1.0,
                                                          16, st)) / 1e3 for _ in range(3)]
        print("local_tail %d, no profiler: forward solve %s ms" % (local, " ".join("%.2f" % t for t in ts)))
    lib.gode_set_option(b"local_tail", 1)
    lib.gode_prof_destroy(prof)


if __name__ == "__main__":
    main()
