"""A/B of the run-time option diag_rows - or, with --option diag_last, of that option under diag_rows 1 - on the
benchmark's training step, in ONE process.

The step is bench.py's (R-MAT 2^20 rows / 10 M edges, d = 128, ODEGCN3 rk4 16 steps, adjoint backward, Adam; one GPU).
The option is set to 1, 0, 1, 0, 1 in turn; each reading is one warm-up step and three timed steps between device
synchronisations (parallel.run_timed, the helper bench.py times with).  Option 0 issues the launches of the code before
the option existed (the forward solve's products with A and the adjoint's products with A^T on their full record lists,
no row stored by the dense launch or by the launch that forms dZ in their place), so the 0 readings are the yardstick; a gain counts when every 1 reading beats every 0 reading and the mean gap is at
least three times the spread among readings of the same setting (--min-ratio; diag_last was held to five times).
diag_last 0 likewise issues the launches of the code before that option: the last stage of every forward rk4 step on A's
full list.  local_tail 0 (under diag_rows 1 and diag_last 1): every row through every dense launch of the forward solve, no
tail launch; adjoint_tail 0 (under diag_rows 1): every row through Gf and Sp(g) of the adjoint solve's forward recompute, no
tail launch there; --set holds further options fixed over all readings (local_tail_blocks, overlap).

    python tools/diag_rows_ab.py [--option diag_rows] [--scale 20] [--edges 10000000] [--ode-steps 16] [--steps 3] [--warmup 1]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--nfeat", type=int, default=128)
    ap.add_argument("--nclass", type=int, default=16)
    ap.add_argument("--ode-steps", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--order", default="1,0,1,0,1", help="settings of the option, one reading each")
    ap.add_argument("--option", default="diag_rows", choices=["diag_rows", "diag_last", "local_tail", "adjoint_tail"])
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE",
                    help="another option held fixed over all readings (e.g. local_tail_blocks=128, overlap=0)")
    ap.add_argument("--min-ratio", type=float, default=3.0, help="mean gap over same-setting spread that counts as a gain")
    args = ap.parse_args()
    from graph_odenet_amd import _lib, models, parallel
    from graph_odenet_amd.optim import Adam
    from graph_odenet_amd.synth import rmat_graph
    lib = _lib.load()
    assert torch.cuda.is_available(), "diag_rows_ab.py needs a GPU"
    dev = torch.device("cuda", 0)
    g = rmat_graph(args.scale, args.edges, seed=0, device=dev)
    g.transpose()
    n = g.n_rows
    gen = torch.Generator(device=dev).manual_seed(1000)
    x = torch.randn(n, args.nfeat, generator=gen, device=dev)
    labels = torch.randint(0, args.nclass, (n,), generator=gen, device=dev)
    idx_train = torch.randperm(n, generator=gen, device=dev)[: n // 10]
    torch.manual_seed(42)
    model = models.ODEGCN3(nfeat=args.nfeat, nhid=args.hidden, nclass=args.nclass, dropout=0.5,
                           method="rk4", step_size=1.0 / args.ode_steps).to(dev)
    opt = Adam(model.parameters(), lr=0.01, weight_decay=5e-4)

    def step():
        model.train()
        opt.zero_grad(set_to_none=False)
        out = model(x, g)
        loss = torch.nn.functional.nll_loss(out[idx_train], labels[idx_train])
        loss.backward()
        opt.step()
        return loss

    name = args.option.encode()
    old = lib.gode_get_option(name)
    fixed = {kv.split("=")[0].encode(): int(kv.split("=")[1]) for kv in args.set}
    old_fixed = {k: lib.gode_get_option(k) for k in fixed}
    readings = []
    try:
        for k, v in fixed.items():
            assert lib.gode_set_option(k, v) == 0 and lib.gode_get_option(k) == v, k
        for _ in range(2):                       # both settings' kernels loaded before the first reading
            for v in (1, 0):
                assert lib.gode_set_option(name, v) == 0
                step()
        torch.cuda.synchronize()
        for v in [int(t) for t in args.order.split(",")]:
            assert lib.gode_set_option(name, v) == 0 and lib.gode_get_option(name) == v
            elapsed, loss = parallel.run_timed(step, args.steps, args.warmup, dev)
            ms = 1e3 * elapsed / args.steps
            readings.append((v, ms))
            print("%s %d: %8.2f ms/step   (loss %.5f)" % (args.option, v, ms, float(loss)), flush=True)
    finally:
        lib.gode_set_option(name, old)
        for k, v in old_fixed.items():
            lib.gode_set_option(k, v)
    on = [ms for v, ms in readings if v == 1]
    off = [ms for v, ms in readings if v == 0]
    res = {"readings": [{args.option: v, "ms_per_step": round(ms, 2)} for v, ms in readings]}
    if fixed:
        res["fixed"] = {k.decode(): v for k, v in fixed.items()}
    if on and off:
        gap = sum(off) / len(off) - sum(on) / len(on)
        spread = max(max(on) - min(on), max(off) - min(off))
        res.update({"mean_on_ms": round(sum(on) / len(on), 2), "mean_off_ms": round(sum(off) / len(off), 2),
                    "gap_ms": round(gap, 2), "same_setting_spread_ms": round(spread, 2),
                    "every_on_beats_every_off": max(on) < min(off),
                    "gap_at_least_%gx_spread" % args.min_ratio: gap >= args.min_ratio * spread})
    res["graph"] = {str(k): v for k, v in g.__dict__.get("_tuned_info", {}).items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
