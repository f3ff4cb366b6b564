#!/usr/bin/env python3
"""bench.py — full-graph ODE-GCN forward+backward steps/sec at 64 RK4 evals (BASELINE.json metric).

Workload (config C5 of SURVEY.md §8(d), the one the metric is quoted on; fits one GPU):
  synthetic R-MAT graph, 2^20 nodes / 10 M directed edges (+ self loops, duplicates removed),
  A_hat = D^-1 (A + I) fp32, features ~ N(0,1) 128-d, hidden 128, 16 classes, dropout 0.5,
  ODEGCN3 shape (GCN/models.py:204-218): gc1 -> relu -> dropout -> ODEBlock(rk4 3/8 rule,
  16 steps x 4 stages = 64 f-evals on [0,1]) -> gc3 -> log_softmax -> NLL on 10 % of the nodes,
  adjoint backward (64 recomputed f-evals + 64 VJPs), Adam(lr .01, wd 5e-4) step
  (GCN/train_res.py:63-79,126-127).  One "step" = that whole pass over one graph.

Multi-GPU (--gpus N): launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`, or bare as
`python bench.py --gpus N`, which starts the N ranks itself as fresh child processes before any GPU call
(graph_odenet_amd/launch.py).  Every rank owns an independent R-MAT graph (seed = rank), i.e. a batch of N graphs sharded
one per GPU; the only exchange step is the RCCL all-reduce of the gradients per step.  scaling = "weak";
value = N*K / max-over-ranks time.  Under N > 1 and --full the line also carries the two other multi-GPU workloads of
SURVEY 8(e),
measured after (outside) the timed region: `secondary.qc_data_parallel` (C4: batches of 20 molecules per rank, the 57 MB
bucketed gradient exchange, graphs/s; tools/qc_bench.py) and `secondary.strong_scaling` (the SAME C5 graph row-partitioned
over the ranks, one all-gather per aggregation; tools/partition_bench.py), and `rccl_ranks` = the ranks that answered a
checked all-reduce of 1.0.  With fewer GPUs than ranks (rehearsal on a one-GPU box) the ranks share the GPUs and exchange
over gloo; `backend` says which.

Prints ONE JSON line on rank 0, the contract line.  A plain run does only what that line's headline figure
needs: set-up, warm-up, the timed steps, the line.  Everything else is measured under `--full` only: `roofline` (SpMM
main kernel, HIP events recorded around every launch of the timed region by libgraphode's profiler hook),
`roofline_dense`, `cpu_baseline` (the oracle timed on the host cores, bounded sample, rank 0, N=1 only) and the
`secondary` block (N = 1: the other BASELINE.json configurations and the extra step readings; N > 1: the two other
multi-GPU workloads above).

`--dump-outputs DIR` writes what the timed path computed in its last step, right after the timed region (rank 0):
`loss.npy`, a fixed sample of the rows of the log-probabilities (`log_probs_sample.npy`, row ids in
`log_probs_sample_rows.npy`), and every parameter after the Adam update and its gradient (`param.<name>.npy`,
`grad.<name>.npy`), float32 (the row ids float64).  The inputs depend on the arguments alone, so two builds can be
compared file by file.
"""
import argparse
import ctypes
import json
import os
import sys
import time

# graph_odenet_amd/hipgraph.py: replayed memset nodes need the HIP runtime's graph fast path off (read at runtime
# initialisation, which torch.cuda.set_device below triggers); no measurable cost on the captured solves
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F32_PEAK_TFLOPS = 157.3   # same guide, "Matrix cores": f32-input MFMA = the fp32 vector rate


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=int, default=20, help="log2(nodes) of the R-MAT graph")
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--nfeat", type=int, default=128)
    ap.add_argument("--nclass", type=int, default=16)
    ap.add_argument("--ode-steps", type=int, default=16, help="rk4 steps on [0,1] (4 evals each)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline figure: rooflines, CPU baseline, secondary block")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32, rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-evals", type=int, default=4, help="f-evals in the CPU-baseline sample (median is used)")
    ap.add_argument("--force-dist", action="store_true",
                    help="rehearsal: initialise RCCL and run the collectives of the multi-GPU path with a single rank")
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the step times of the other BASELINE.json configurations (Cora / Pubmed / Citeseer-GAT / QC)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the untimed-by-contract extras: per-f-eval times and the 256-eval reading (N = 1); the QC "
                         "data-parallel and strong-scaling entries (N > 1)")
    ap.add_argument("--backend", choices=["auto", "nccl", "gloo"], default="auto",
                    help="auto: nccl (= RCCL) with a GPU per rank, else gloo with the ranks sharing the GPUs (rehearsal)")
    ap.add_argument("--configs-timeout", type=float, default=420.0, help="seconds allowed to tools/config_bench.py (N = 1)")
    ap.add_argument("--qc-steps", type=int, default=30, help="timed steps of secondary.qc_data_parallel (N > 1)")
    ap.add_argument("--secondary-timeout", type=float, default=420.0,
                    help="N > 1: seconds after which the line is printed without the secondary entries still running")
    return ap.parse_args()


def cpu_baseline(args, graph_cpu, sd, x_cpu):
    """Oracle (kind 'port') on the host cores: a bounded sample of the same workload, scaled."""
    from oracle import layers_ref as R
    n = graph_cpu["n"]
    adj = torch.sparse_coo_tensor(torch.stack([graph_cpu["r"], graph_cpu["c"]]), graph_cpu["v"], (n, n))
    adj = adj.coalesce()
    p = [sd["gc2.odefunc.norm1.weight"], sd["gc2.odefunc.norm1.bias"], sd["gc2.odefunc.gc1.weight"],
         sd["gc2.odefunc.gc1.bias"]]
    with torch.no_grad():
        h = torch.relu(R.graph_convolution(x_cpu, adj, sd["gc1.weight"], sd["gc1.bias"]))
        R.odefunc(torch.tensor(0.1), h, adj, *p)                      # warm-up
        ts = []
        for i in range(args.cpu_evals):
            t0 = time.perf_counter()
            R.odefunc(torch.tensor(0.1 * i), h, adj, *p)
            ts.append(time.perf_counter() - t0)
        t_f = sorted(ts)[len(ts) // 2]
    # one f-eval with its VJP (what every adjoint stage costs)
    pg = [q.clone().requires_grad_(True) for q in p]
    hg = h.clone().requires_grad_(True)
    t0 = time.perf_counter()
    out = R.odefunc(torch.tensor(0.3), hg, adj, *pg)
    out.backward(torch.ones_like(out))
    t_fb = time.perf_counter() - t0
    nfe = 4 * args.ode_steps
    est = nfe * t_f + nfe * t_fb            # forward solve + adjoint solve (first/last layers ignored)
    return {"value": 1.0 / est, "unit": "steps/s", "cores": torch.get_num_threads(), "kind": "port",
            "host_cpu_count": os.cpu_count(), "ms_per_feval": round(1e3 * t_f, 1),
            "sample": "1 warm-up + %d ODEfunc f-evals (median %.2f s) + 1 f-eval with VJP (%.2f s) on the same 2^%d-node "
                      "graph, scaled to %d fwd + %d adjoint evals per step" % (args.cpu_evals, t_f, t_fb, args.scale, nfe, nfe)}


def secondary(args, model, x, g, step, barrier):
    """SURVEY 8(d) extras, measured after (outside) the timed region: per-f-eval times of the ODE block and the
    "64 ODE steps" reading (64 rk4 steps = 256 f-evals forward)."""
    blk = model.gc2
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    with torch.no_grad():
        h = torch.relu(model.gc1(x, g))
    h.requires_grad_(True)
    blk(h, g).sum().backward()                                      # warm-up
    ev[0].record()
    y = blk(h, g)
    ev[1].record()
    y.backward(torch.ones_like(y))
    ev[2].record()
    torch.cuda.synchronize()
    nfe = 4 * args.ode_steps
    out = {"ms_per_feval_forward": round(ev[0].elapsed_time(ev[1]) / nfe, 4),
           "ms_per_adjoint_stage": round(ev[1].elapsed_time(ev[2]) / nfe, 4),
           "note": "forward f-eval = fused GN+time+GEMM + SpMM; adjoint stage = recomputed f-eval + VJP + weight grads"}
    old = blk.step_size
    blk.step_size = old / 4.0
    try:
        step()
        barrier()
        t0 = time.perf_counter()
        step()
        barrier()
        out["steps_per_s_at_256_evals"] = round(1.0 / (time.perf_counter() - t0), 4)
    finally:
        blk.step_size = old
    # the same step with every dense product on the exact-fp32 MFMA kernels (gemm_split 0, wgrad_split 0), for the A/B
    # against the default (bf16-piece kernels for the weight gradient and the <= 2-term forward launches)
    from graph_odenet_amd import _lib
    lib = _lib.load()
    names = (b"gemm_split", b"wgrad_split", b"fwd_pc", b"bwd_pc", b"bwd_wgrad", b"y2_colsum")
    was = [lib.gode_get_option(k) for k in names]

    def timed(settings, reps=2):
        try:
            for k, v in zip(names, settings):
                if lib.gode_set_option(k, v) != 0:
                    return None
            step()
            barrier()
            t0 = time.perf_counter()
            for _ in range(reps):
                step()
            barrier()
            return round(reps / (time.perf_counter() - t0), 4)
        finally:
            for k, v in zip(names, was):
                lib.gode_set_option(k, v)
    # same box, same process, back to back: the round-2 kernel selection (VJP and 3-4 term forward on the fp32-MFMA
    # kernels, <= 2-term forward on gn_gemm_fwd_split_kernel), every dense product on the fp32-MFMA kernels, and the
    # default again (the first and last figure bracket the drift of the box)
    out["steps_per_s_default_kernels"] = timed(was)
    out["steps_per_s_with_bias_gradient_from_a_pass_over_dZ"] = timed((was[0], was[1], was[2], was[3], was[4], 0))   # before round 4's SpMM epilogue sums
    out["steps_per_s_with_separate_vjp_and_weight_gradient_launches"] = timed((was[0], was[1], was[2], was[3], 0, was[5]))   # round 3
    out["steps_per_s_with_round2_dense_kernels"] = timed((2, was[1], 0, 0, 0, was[5]))
    out["steps_per_s_with_fp32_mfma_dense_kernels_only"] = timed((0, 0, 0, 0, 0, was[5]))
    out["steps_per_s_default_kernels_again"] = timed(was)
    return out


BF16_PEAK_TFLOPS = 2500.0     # dense bf16 MFMA peak (MI355X_MICROARCH.md, "Peak BF16/FP16 MFMA ~2.5 PF dense")
FAMILY = {1: ("forward S = [t|GN(x)]W", 2), 2: ("VJP dx = GN'(x)^T dS W1^T", 3), 3: ("weight gradient dW = [1|GN(x)]^T dS", 2),
          4: ("VJP + weight gradient in one pass (2 products)", 3)}
FAMILY_PRODUCTS = {1: 1, 2: 1, 3: 1, 4: 2}            # N x d x d products a launch of the family forms
KERNEL = {(1, 0): "gn_gemm_fwd_kernel<8,4> (fp32 MFMA)", (1, 1): "gn_gemm_fwd_split_kernel (bf16 pieces)",
          (1, 2): "gn_gemm_fwd_pc_kernel (bf16 pieces, producer/consumer)",
          (2, 0): "gn_gemm_bwd_kernel<8,4> (fp32 MFMA)",
          (2, 2): "gn_gemm_bwd_pc_kernel (bf16 pieces, producer/consumer)",
          (3, 0): "wgrad_kernel<8,4> (fp32 MFMA)", (3, 2): "wgrad_split_kernel (bf16 pieces, producer/consumer)",
          (4, 2): "gn_gemm_bwd_wgrad_pc_kernel (bf16 pieces, one producer group, transposed LDS reads)"}


def dense_table(lib, cnt, ms, dd, rr, xx, kk, n, hidden, flop, nd4):
    """roofline_dense: launches grouped by (family, kernel form, extra operand arrays); see the comment at the call."""
    groups = {}
    for i in range(max(cnt, 0)):
        fam, form = kk[i] & 0xff, kk[i] >> 8
        if fam in FAMILY and dd[i] == hidden and rr[i] == n:
            groups.setdefault((fam, form, int(xx[i])), []).append(ms[i])
    if not groups:
        return None
    out = {"bound": "mfma", "peak": MFMA_F32_PEAK_TFLOPS, "peak_bf16": BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
           "flop_per_launch": flop, "kernels": {}, "families": {},
           "note": "kernels: one entry per (kernel that ran, extra N x d operand arrays beyond the one-term launch: stage "
                   "terms, x_out, pre-terms); frac_fp32_equiv = 2*N*d*d flop / time / 157.3 TFLOP/s; frac_of_unit = the "
                   "same for fp32-MFMA kernels, 8 piece products x 2*N*d*d / time / 2 500 TFLOP/s for the bf16-piece "
                   "kernels.  families: launch-weighted mean over every launch of the family in the timed region."}
    fam_tot = {}
    for (fam, form, extra), v in sorted(groups.items()):
        avg = sum(v) / len(v)
        byts = (FAMILY[fam][1] + extra) * nd4
        eq = FAMILY_PRODUCTS[fam] * flop / (avg * 1e-3) / 1e12
        unit = eq / MFMA_F32_PEAK_TFLOPS if form == 0 else 8 * eq / BF16_PEAK_TFLOPS
        out["kernels"]["%s, +%d arrays" % (KERNEL.get((fam, form), "family %d form %d" % (fam, form)), extra)] = {
            "launches_timed": len(v), "avg_launch_ms": round(avg, 4), "achieved": round(eq, 1),
            "frac_fp32_equiv": round(eq / MFMA_F32_PEAK_TFLOPS, 4), "frac_of_unit": round(unit, 4),
            "algorithmic_bytes_per_launch": int(byts), "hbm_GBps": round(byts / (avg * 1e-3) / 1e9, 1)}
        t = fam_tot.setdefault(fam, [0.0, 0])
        t[0] += sum(v); t[1] += len(v)
    for fam, (tot, c) in fam_tot.items():
        avg = tot / c
        out["families"][FAMILY[fam][0]] = {"launches_timed": c, "avg_launch_ms": round(avg, 4),
                                           "frac_fp32_equiv": round(FAMILY_PRODUCTS[fam] * flop / (avg * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4)}
    return out


def multi_gpu_secondary(args, dev, rank, world, backend):
    """SURVEY 8(e)'s two other multi-GPU workloads, after the timed region; every rank calls this (collectives inside).
    An exception on every rank becomes an `error` entry; a hang is the watchdog's business (main)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    out = {}
    small = args.scale < 20            # rehearsal sizes: keep the QC leg short too
    try:
        import qc_bench
        out["qc_data_parallel"] = qc_bench.run(dev, rank, world, backend, "MPNN_ENN_K_Set2Set",
                                               steps=max(2, args.qc_steps if not small else min(args.qc_steps, 4)),
                                               warmup=3 if not small else 1, batch_size=20)
    except Exception as e:
        import traceback
        out["qc_data_parallel"] = {"error": "%s: %s" % (type(e).__name__, e), "where": traceback.format_exc()[-1500:]}
    torch.cuda.empty_cache()
    try:
        import partition_bench
        out["strong_scaling"] = partition_bench.run(dev, rank, world, backend, args.scale, args.edges, args.nfeat,
                                                    args.hidden, args.nclass, args.ode_steps, steps=max(1, min(args.steps, 2)),
                                                    warmup=1)
    except Exception as e:
        import traceback
        out["strong_scaling"] = {"error": "%s: %s" % (type(e).__name__, e), "where": traceback.format_exc()[-1500:]}
    torch.cuda.empty_cache()
    return out


DUMP_SAMPLE_ROWS = 65536          # rows of the N x nclass log-probabilities written by --dump-outputs (4 MB at 16 classes)
DUMP_SAMPLE_BYTES = 32 << 20      # ... and never more than this


def dump_outputs(out_dir, loss, log_probs, model):
    """--dump-outputs: the last timed step's loss, a fixed sample of its output rows (the same rows for the same
    arguments), and the parameters after the update with their gradients, as .npy files (float32; the row ids float64)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)

    def save(name, t, dtype=torch.float32):
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().to("cpu", dtype).numpy())
    n, c = log_probs.shape
    k = min(n, DUMP_SAMPLE_ROWS, max(1, DUMP_SAMPLE_BYTES // (4 * c)))
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:k].sort().values
    save("loss", loss.reshape(1))
    save("log_probs_sample", log_probs[rows.to(log_probs.device)])
    save("log_probs_sample_rows", rows, torch.float64)
    for name, p in model.named_parameters():
        save("param." + name, p)
        if p.grad is not None:
            save("grad." + name, p.grad)


def full_measurements(args, lib, prof, cap, g, n, world, model, x, step, barrier, other_configs):
    """`--full` only, after the timed region: the rooflines from the profile of the timed steps, and (N = 1) the
    secondary block - extra steps with other settings, the dense kernels alone, the other configurations."""
    # ---- roofline of the dominant kernel (SpMM main kernel at d = hidden) and of the dense kernels --------------
    ms = (ctypes.c_float * cap)()
    dd = (ctypes.c_int64 * cap)()
    rr = (ctypes.c_int64 * cap)()
    xx = (ctypes.c_int64 * cap)()
    kk = (ctypes.c_int32 * cap)()
    cnt = lib.gode_prof_read(prof, ms, dd, rr, xx, cap)
    lib.gode_prof_kinds(prof, kk, cap)
    from graph_odenet_amd.gcn_ode import tuned_graph
    g_run = tuned_graph(g, args.hidden)[0]        # the (possibly renumbered) graph the ODE block ran on; cached by the solve
    sel = [i for i in range(max(cnt, 0)) if kk[i] == 0 and dd[i] == args.hidden
           and rr[i] in (g_run.n_items, g_run.transpose().n_items)]
    lib.gode_prof_destroy(prof)
    roof = None
    nd4 = n * args.hidden * 4
    if sel:
        tot_ms = sum(ms[i] for i in sel)
        avg_ms = tot_ms / len(sel)
        # B_alg = nnz*(4+4+4d) + (N+1)*4 + N*d*4 per launch; `frac` prices exactly that.  The fused
        # epilogue of a launch also reads / writes further N x d arrays (RK combine terms, adjoint cotangent terms,
        # the masked output): those bytes are reported separately as frac_with_epilogue_operands.
        b_alg = g.algorithmic_bytes(args.hidden)
        tot_bytes = sum(b_alg + xx[i] * nd4 for i in sel)
        ach = b_alg / (avg_ms * 1e-3) / 1e9
        traffic = None
        tf = os.path.join(ROOT, "profiles", "spmm_traffic.json")
        if os.path.exists(tf) and (args.scale, args.edges, args.hidden) == (20, 10_000_000, 128):   # measured on THIS workload only
            try:
                traffic = json.load(open(tf)).get("hbm_bytes_per_launch")
            except Exception:
                traffic = None
        b_min = g.nnz * 8 + (n + 1) * 4 + 2 * nd4            # SURVEY 8(d) compulsory lower bound of the plain product
        roof = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic,
                "kernel": "spmm_vec4_kernel<%d>" % (args.hidden // 4), "launches_timed": len(sel),
                "avg_launch_ms": round(avg_ms, 4), "algorithmic_bytes_per_launch": b_alg,
                "compulsory_bytes_per_launch": b_min,
                "frac_with_epilogue_operands": round(tot_bytes / (tot_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "epilogue_operand_arrays_per_launch": round(sum(xx[i] for i in sel) / len(sel), 3),
                "node_order": dict(g.__dict__["_tuned_info"][(args.hidden, "auto")])}
    # dense kernels: one entry per (family, kernel that ran, number of extra N x d operand arrays).  Every launch does
    # 2*N*d*d fp32-equivalent flop.  Two fractions:
    #   frac_fp32_equiv = that rate / the 157.3 TFLOP/s fp32 matrix peak - comparable across kernels, NOT a roofline
    #                     fraction of the unit a bf16-piece kernel runs on;
    #   frac_of_unit    = fp32 kernels: the same number; bf16-piece kernels: the 8 piece products actually issued
    #                     (8 x 2*N*d*d flop) / the 2 500 TFLOP/s dense bf16 matrix peak.
    # Durations are AS SCHEDULED: in the adjoint the VJP runs beside the weight gradient / next forward product on a
    # second stream (alone_single_stream below: the same launches with that schedule off).
    flop = 2.0 * n * args.hidden * args.hidden
    dense = dense_table(lib, cnt, ms, dd, rr, xx, kk, n, args.hidden, flop, nd4)

    extras = None
    if world == 1 and not args.no_secondary:
        extras = secondary(args, model, x, g, step, barrier)
        # the dense kernels ALONE: one more step with the two-stream adjoint schedule off (outside the timed region), so
        # that roofline_dense can be read both ways - as scheduled (above) and per kernel
        if dense is not None and lib.gode_get_option(b"overlap") == 1:
            cap2 = 8 * 4 * args.ode_steps + 96
            prof2 = lib.gode_prof_create(cap2)
            lib.gode_set_option(b"overlap", 0)
            try:
                lib.gode_prof_enable(prof2)
                step()
                barrier()
                lib.gode_prof_enable(None)
                ms2, dd2, rr2, xx2 = ((ctypes.c_float * cap2)(), (ctypes.c_int64 * cap2)(), (ctypes.c_int64 * cap2)(),
                                      (ctypes.c_int64 * cap2)())
                kk2 = (ctypes.c_int32 * cap2)()
                c2 = lib.gode_prof_read(prof2, ms2, dd2, rr2, xx2, cap2)
                lib.gode_prof_kinds(prof2, kk2, cap2)
                alone = dense_table(lib, c2, ms2, dd2, rr2, xx2, kk2, n, args.hidden, flop, nd4)
                dense["alone_single_stream"] = {k: {"avg_launch_ms": v["avg_launch_ms"], "frac_fp32_equiv": v["frac_fp32_equiv"],
                                                    "frac_of_unit": v["frac_of_unit"], "hbm_GBps": v["hbm_GBps"]}
                                                for k, v in (alone or {}).get("kernels", {}).items()}
            finally:
                lib.gode_set_option(b"overlap", 1)
                lib.gode_prof_destroy(prof2)
        if other_configs is not None:
            extras["other_configs"] = other_configs
    return roof, dense, extras


def main():
    args = parse()
    from graph_odenet_amd import launch
    if launch.needs_self_launch(args.gpus):
        # bare `python bench.py --gpus N`: start the N ranks as fresh children BEFORE this process touches the GPU, relay
        # their output (rank 0 prints the JSON line) and leave with their exit code
        sys.exit(launch.self_launch(__file__, sys.argv[1:], args.gpus))
    other_configs = None
    if args.full and int(os.environ.get("WORLD_SIZE", "1")) == 1 and not args.no_configs and not args.no_secondary:
        # The other BASELINE.json configurations (parity-test cases) with their CPU legs, timed on this box by
        # tools/config_bench.py in a CHILD process that runs to completion BEFORE this process makes its first GPU call
        # (a process that has initialised the GPU starts no further programs on this pool).  A fresh process also keeps
        # the C4 leg's HIP-graph captures of arbitrary autograd away from the process that prints the contract line.
        import subprocess
        try:
            assert not torch.cuda.is_initialized()
            cp = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "config_bench.py"), "--one-line"],
                                capture_output=True, text=True, timeout=args.configs_timeout)
            lines = [l for l in cp.stdout.splitlines() if l.startswith("{")]
            if cp.returncode != 0 or not lines:
                raise RuntimeError("config_bench.py rc %d: %s" % (cp.returncode, (cp.stderr or cp.stdout)[-400:]))
            other_configs = json.loads(lines[-1])
        except Exception as e:
            other_configs = {"error": "%s: %s" % (type(e).__name__, e)}
    import torch.distributed as dist
    if args.force_dist and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        rank, local_rank, world, backend = 0, 0, 1, "nccl"
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    else:
        rank, local_rank, world, dev, backend = launch.init_ranks(args.backend)      # includes the checked all-reduce of 1.0
    if world != args.gpus and rank == 0:
        print("bench.py: --gpus %d but WORLD_SIZE=%d; reporting n_gpus=%d" % (args.gpus, world, world), file=sys.stderr)
    use_dist = world > 1 or args.force_dist

    from graph_odenet_amd import _lib, models, ops
    from graph_odenet_amd import parallel
    from graph_odenet_amd.parallel import GradBucket, broadcast_parameters
    parallel.FORCE_COLLECTIVES = bool(args.force_dist)
    from graph_odenet_amd.synth import rmat_graph
    lib = _lib.load()

    # ---- inputs: resident in HBM before the timed region ------------------------------------
    g = rmat_graph(args.scale, args.edges, seed=rank, device=dev)
    g.transpose()                                   # CSR-by-source for the backward pass, built once
    n = g.n_rows
    gen = torch.Generator(device=dev).manual_seed(1000 + rank)
    x = torch.randn(n, args.nfeat, generator=gen, device=dev)
    labels = torch.randint(0, args.nclass, (n,), generator=gen, device=dev)
    idx_train = torch.randperm(n, generator=gen, device=dev)[: n // 10]

    torch.manual_seed(42)
    model = models.ODEGCN3(nfeat=args.nfeat, nhid=args.hidden, nclass=args.nclass, dropout=0.5,
                           method="rk4", step_size=1.0 / args.ode_steps).to(dev)
    broadcast_parameters(model, 0)
    from graph_odenet_amd.optim import Adam
    opt = Adam(model.parameters(), lr=0.01, weight_decay=5e-4)        # torch.optim.Adam's update as one launch (csrc/mlp.hip)
    bucket = GradBucket(model)
    sd_cpu = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()} if args.full else None
    last_out = [] if args.dump_outputs and rank == 0 else None

    def step():
        model.train()
        opt.zero_grad(set_to_none=False)
        out = model(x, g)
        loss = torch.nn.functional.nll_loss(out[idx_train], labels[idx_train])
        loss.backward()
        bucket.allreduce_mean()
        opt.step()
        if last_out is not None:
            last_out[:] = [out.detach()]
        return loss

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    model.nfe = 0
    if args.full:
        cap = args.steps * (8 * 4 * args.ode_steps + 32) + 64
        prof = lib.gode_prof_create(cap)
        lib.gode_prof_enable(prof)
    # exactly `steps` steps between barrier + synchronize on both sides, MAX over ranks (parallel.run_timed: the same
    # helper the world_size-2 gloo test drives)
    elapsed, loss = parallel.run_timed(step, args.steps, 0, dev)
    if args.full:
        lib.gode_prof_enable(None)
    nfe_per_step = model.nfe / max(args.steps, 1)
    if last_out is not None:
        dump_outputs(args.dump_outputs, loss, last_out[0], model)
    roof = dense = extras = None
    if args.full:
        roof, dense, extras = full_measurements(args, lib, prof, cap, g, n, world, model, x, step, barrier, other_configs)

    res = None
    if rank == 0:
        res = {
            "metric": "full-graph ODE-GCN forward+backward steps/sec at 64 RK4 evals",
            "value": round(world * args.steps / elapsed, 4), "unit": "steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 2),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "RMAT scale-%d / %d edges (+self loops, dedup) row-normalised, d=%d, "
                                   "ODEGCN3 rk4(3/8) %d steps = %d f-evals fwd, adjoint bwd, Adam; one graph per GPU"
                                   % (args.scale, args.edges, args.hidden, args.ode_steps, 4 * args.ode_steps),
                       "nodes": n, "nnz": g.nnz, "nfeat": args.nfeat, "hidden": args.hidden,
                       "nclass": args.nclass, "nfe_per_step": nfe_per_step,
                       "parallelism": "dp%d (one graph per rank, 1 gradient all-reduce/step)" % world},
            "loss": round(float(loss.detach()), 5),
        }
        if args.full:
            res["roofline"] = roof
            res["roofline_dense"] = dense
        if use_dist:
            # ranks that answered the checked all-reduce of 1.0 at start-up (launch.init_ranks), and what carried it:
            # "nccl" = RCCL, one GPU per rank; "gloo" = rehearsal, the ranks share the GPUs of a smaller box
            res["rccl_ranks"] = dist.get_world_size()
            res["backend"] = backend
        if extras is not None:
            res["secondary"] = extras
        if args.full and world == 1 and not args.no_cpu_baseline:
            rp = g.rowptr.to(torch.int64)
            rows = torch.repeat_interleave(torch.arange(n, device=dev), rp[1:] - rp[:-1]).cpu()
            gc = {"n": n, "r": rows, "c": g.col.to(torch.int64).cpu(), "v": g.val.cpu()}
            res["cpu_baseline"] = cpu_baseline(args, gc, sd_cpu, x.cpu())

    if args.full and world > 1 and not args.no_secondary:
        # The two other multi-GPU workloads run AFTER the contract measurement is complete.  They are collective code
        # that may stall on a node this build has never seen: a watchdog prints the line without them (and ends the
        # process, on every rank) rather than let a secondary number take the contract line down.
        import threading
        lock, done = threading.Lock(), [False]

        def give_up():
            with lock:
                if done[0]:
                    return
                done[0] = True
                if rank == 0:
                    res["secondary"] = {"error": "qc_data_parallel / strong_scaling did not finish within %.0f s"
                                                 % args.secondary_timeout}
                    print(json.dumps(res), flush=True)
                os._exit(0)
        dog = threading.Timer(args.secondary_timeout + (0.0 if rank == 0 else 15.0), give_up)
        dog.daemon = True
        dog.start()
        del model, opt, bucket, x, labels, idx_train, step
        g = g_run = None
        torch.cuda.empty_cache()
        sec = multi_gpu_secondary(args, dev, rank, world, backend)
        with lock:
            dog.cancel()
            if done[0]:
                return
            done[0] = True
        if rank == 0:
            res["secondary"] = sec
    if rank == 0:
        print(json.dumps(res), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
