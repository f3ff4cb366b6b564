#!/usr/bin/env python3
"""Same-process A/B of the dense kernel variants at 2^20 x 128 (box-to-box spread is +-10 %, so variants are timed
interleaved in ONE process: median of `--reps` rounds, each round timing every variant once).

--diag: the forms of the forward launch that also close diagonal-only rows (gode_gn_time_gemm_diag_f32, 1-3 terms;
gode_gn_time_gemm_diag_aux_f32, 4 terms + closing combination) against their plain siblings, the same way.  Flags as on the
benchmark graph: 55.0 % of the rows flagged (random rows, a_ii in .25 .. .85), 45.4 % of all rows also skipped; the bytes a
form adds (+) and saves (-) per launch are printed beside the difference."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from graph_odenet_amd import _lib, ops  # noqa: E402


def diag_forms(a, lib, dev, n, d):
    gen = torch.Generator(device=dev).manual_seed(3)
    X, K1, K2, K3, S, OUT = [torch.randn(n, d, generator=gen, device=dev) for _ in range(6)]
    W = torch.randn(d + 1, d, generator=gen, device=dev) / d ** 0.5
    gam, bet = torch.rand(d, generator=gen, device=dev) + 0.5, torch.rand(d, generator=gen, device=dev) - 0.5
    bias = torch.randn(d, generator=gen, device=dev)
    u = torch.rand(n, generator=gen, device=dev)
    diag = torch.where(u < 0.55, 0.25 + 0.6 * torch.rand(n, generator=gen, device=dev), torch.zeros(n, device=dev))
    skip = torch.where(u < 0.454, diag, torch.zeros(n, device=dev))
    nf, ns = int((diag != 0).sum()), int((skip != 0).sum())
    T = [(1.0, X), (0.1, K1), (-0.1, K2), (0.1, K3)]
    coefs = (ctypes.c_float * 8)(1.0, 0.0125, 0.0375, 0.0375, 0, 0, 0, 0)
    p, sp = _lib.ptr, _lib.stream_ptr

    def call(fn, terms, *more):
        lc = _lib.lincomb(terms)
        _lib.check(fn(ctypes.byref(lc), n, d, 32, 1e-5, p(gam), p(bet), p(W), d, 1, 0.3, p(S), *more, sp()), "dense launch")

    def diag_call(terms):
        taken = ctypes.c_int32(0)
        call(lib.gode_gn_time_gemm_diag_f32, terms, p(diag), p(skip), p(bias), p(OUT), ctypes.byref(taken))
        assert taken.value == 1

    def last_call():
        taken = ctypes.c_int32(0)
        call(lib.gode_gn_time_gemm_diag_aux_f32, T, coefs, p(OUT), 0.0078125, p(diag), p(skip), p(bias), ctypes.byref(taken))
        assert taken.value == 1

    row = 4 * d
    # bytes against the plain sibling: 8 B of flags per row; 1-3 terms: + K of a flagged row, - S of a skipped row;
    # 4 terms + aux: the flagged row's store replaces its P store, - S of a skipped row
    pairs = [("fwd %d" % k, (lambda k=k: call(lib.gode_gn_time_gemm_f32, T[:k])), (lambda k=k: diag_call(T[:k])),
              8 * n + row * nf, row * ns) for k in (1, 2, 3)]
    pairs.append(("fwd 4+aux", lambda: call(lib.gode_gn_time_gemm_xout_aux_f32, T, None, coefs, p(OUT)), last_call, 8 * n, row * ns))
    res = {name: ([], []) for name, *_ in pairs}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rep in range(a.reps + 1):
        for name, plain, form, _, _ in pairs:
            for which, fn in enumerate((plain, form)):
                fn()
                ev[0].record()
                for _ in range(5):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                if rep:
                    res[name][which].append(ev[0].elapsed_time(ev[1]) / 5)
    print("%d rows, %d flagged, %d of them skipped" % (n, nf, ns))
    print("%-10s %10s %10s %10s %12s %12s" % ("case", "plain ms", "diag ms", "diff us", "+ MB", "- MB"))
    for name, _, _, plus, minus in pairs:
        m = [sorted(v)[len(v) // 2] for v in res[name]]
        print("%-10s %10.4f %10.4f %10.1f %12.1f %12.1f" % (name, m[0], m[1], 1e3 * (m[1] - m[0]), plus / 1e6, minus / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--diag", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, d = 1 << 20, 128
    if a.diag:
        return diag_forms(a, lib, dev, n, d)
    X, K1, K2, K3, Y, OUT, XO, PRE = [torch.randn(n, d, device=dev) for _ in range(8)]
    W = torch.randn(d + 1, d, device=dev) / d ** 0.5
    gam, bet = torch.rand(d, device=dev) + 0.5, torch.rand(d, device=dev) - 0.5
    T = [(1.0, X), (0.1, K1), (-0.1, K2), (0.1, K3)]
    cases = {
        "fwd 1": lambda: ops.gn_time_gemm(T[:1], n, d, 32, 1e-5, gam, bet, W, True, 0.3, out=OUT),
        "fwd 2": lambda: ops.gn_time_gemm(T[:2], n, d, 32, 1e-5, gam, bet, W, True, 0.3, out=OUT),
        "fwd 3": lambda: ops.gn_time_gemm(T[:3], n, d, 32, 1e-5, gam, bet, W, True, 0.3, out=OUT),
        "fwd 4": lambda: ops.gn_time_gemm(T, n, d, 32, 1e-5, gam, bet, W, True, 0.3, out=OUT),
        "fwd 4+xout": lambda: ops.gn_time_gemm(T, n, d, 32, 1e-5, gam, bet, W, True, 0.3, out=OUT, x_out=XO),
        "bwd 1": lambda: ops.gn_time_gemm_bwd(T[:1], n, d, 32, 1e-5, gam, W, True, Y, out=OUT),
        "bwd 2": lambda: ops.gn_time_gemm_bwd(T[:2], n, d, 32, 1e-5, gam, W, True, Y, out=OUT),
        "bwd 1+pre4": lambda: ops.gn_time_gemm_bwd(T[:1], n, d, 32, 1e-5, gam, W, True, Y, out=OUT, out_scale=0.1,
                                                   pre_terms=[(1.0, PRE), (0.1, K1), (0.2, K2), (0.3, K3)]),
        "wgrad 1": lambda: ops.wgrad(T[:1], n, d, 32, 1e-5, gam, bet, Y, True),
    }
    variants = {"round 2": dict(fwd_pc=0, bwd_pc=0), "producer/consumer": dict(fwd_pc=3, bwd_pc=1), "round 2 again": dict(fwd_pc=0, bwd_pc=0)}
    res = {c: {v: [] for v in variants} for c in cases}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rep in range(a.reps + 1):
        for cname, fn in cases.items():
            for vname, opts in variants.items():
                for k, v in opts.items():
                    assert lib.gode_set_option(k.encode(), v) == 0
                fn()
                ev[0].record()
                for _ in range(5):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                if rep:
                    res[cname][vname].append(ev[0].elapsed_time(ev[1]) / 5)
    print("%-12s" % "case" + "".join("%16s" % v for v in variants))
    for c in cases:
        print("%-12s" % c + "".join("%13.4f ms" % sorted(res[c][v])[len(res[c][v]) // 2] for v in variants))


if __name__ == "__main__":
    main()
