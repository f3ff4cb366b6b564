#!/usr/bin/env python3
"""Outputs of the C drivers' entry points (csrc/ode_driver.hip, csrc/gat_driver.hip) on seeded, CPU-generated inputs, for
comparing two builds of the library bit for bit: run it once per build, each in its own process.

  python tools/driver_dump.py --out DIR [--root TREE]            writes every output array to DIR/<name>.npy
  python tools/driver_dump.py --against DIR [--root TREE] [--list FILE]
                                                                  the same calls, every array compared with the one in DIR
                                                                  by numpy.array_equal; prints (and writes to FILE) the list
                                                                  of compared arrays, exit status 1 if one differs

TREE is the checkout whose graph_odenet_amd (and built libgraphode.so) is imported; default: the one this file is in.

Every entry point that runs a launch sequence over a tableau is called by its export name through the binding (_lib), with
the structs and work arrays the fields build, so that the rk4 / dopri5 entry points and the by-method ones are both reached
whichever of them the fields' own members call:
  GCN (gode_gcn_ode_*)  rk4_forward, rk4_forward_save, rk4_adjoint, rk4_backprop (whole interval and step_begin > 0);
                        fixed_forward / _forward_save / _backprop / _adjoint under euler, midpoint and rk4; adams_forward /
                        _adjoint / _forward_save / _backprop at 7 steps; dopri5_step_forward and adaptive_step_forward (they
                        make the stages the sweeps read); dopri5_step_backprop and adaptive_step_backprop under the three codes,
                        first = 0 / 1, with and without kbar_last, with and without a zeroed entry of wk (a dead stage)
  GAT (gode_gat_ode_*)  rk4_forward_save, rk4_backprop, fixed_forward_save / _backprop under the three codes,
                        dopri5_step_backprop and adaptive_step_backprop as above
Shapes, the smallest that reach each route (2 steps unless said):
  gcn-small     300 rows, d = 16: the fused launch-bound route; gcn-multi: the same graph with option small_fused off (the
                multi-launch route below 65 536 rows, merged finish)
  gcn-large128  the 65 600-row uniform graph of tests/test_gpu_driver_launch_order.py at d = 128 (one-pass VJP + weight
                gradient, closing combination once): the fixed-grid entry points; gcn-large64: d = 64, everything
  gat-1x16      600 nodes, one head, d = 16, 1 400 edges; gat-8x8-E900 / gat-8x8-E1400: 8 heads x 8, the H-fold graph below /
                above the 8 192 edges of the raw-logit route
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

T0, T1, N_STEPS, ADAMS_STEPS = 0.0, 1.0, 2, 7
FIXED = ("euler", "midpoint", "rk4")
ADAPTIVE = ("dopri5", "bosh3", "adaptive_heun")


class Recorder:
    def __init__(self, out, against):
        self.out, self.against, self.lines, self.bad = out, against, [], 0
        if out:
            os.makedirs(out, exist_ok=True)

    def __call__(self, name, t):
        torch.cuda.synchronize()
        a = t.detach().cpu().numpy()
        assert np.isfinite(a).all(), name
        if self.out:
            np.save(os.path.join(self.out, name + ".npy"), a)
        if self.against:
            ref = np.load(os.path.join(self.against, name + ".npy"))
            eq = ref.shape == a.shape and ref.dtype == a.dtype and bool(np.array_equal(ref, a))
            self.bad += not eq
            self.lines.append("%-64s %-22s %-8s %s" % (name, "x".join(map(str, a.shape)), a.dtype, "equal" if eq else "DIFFERS"))
        else:
            self.lines.append("%-64s %-22s %-8s written" % (name, "x".join(map(str, a.shape)), a.dtype))
        print(self.lines[-1], flush=True)


def seeded(shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- GCN ------------------------------------------------------------------------------------------------------------------
def uniform_graph(n_rows, dev):
    """tests/test_gpu_driver_launch_order.py: graph - 7 random columns and a self loop per row, row-normalised."""
    from graph_odenet_amd import graph as G
    gen = torch.Generator().manual_seed(65_600)
    rows = torch.arange(n_rows).repeat_interleave(7)
    cols = torch.randint(0, n_rows, (rows.numel(),), generator=gen)
    ar = torch.arange(n_rows)
    key = torch.unique(torch.cat([rows, ar]) * n_rows + torch.cat([cols, ar]))
    r, c = key // n_rows, key % n_rows
    v = 1.0 / torch.bincount(r, minlength=n_rows).to(torch.float32)[r]
    return G.from_coo(r.to(dev), c.to(dev), v.to(dev), n_rows, n_rows, coalesce=False)


class Gcn:
    """The fields of models.ODEfunc(d) on a graph, and the entry points called by name on their structs and work arrays."""

    def __init__(self, g, d, dev):
        from graph_odenet_amd import _lib, gcn_ode, models, odeint as OI
        self.L, self.G, self.lib, self.dev = _lib, gcn_ode, _lib.load(), dev
        torch.manual_seed(7 + d)
        f = models.ODEfunc(d)
        with torch.no_grad():
            f.norm1.weight.uniform_(0.5, 1.5)
            f.norm1.bias.uniform_(-0.5, 0.5)
        self.f = f.to(dev)
        self.f.set_adj(g)
        self.n, self.d = g.n_rows, d
        self.y0, self.a1 = seeded((self.n, d), d).to(dev), seeded((self.n, d), d + 1).to(dev)
        self.fwd, self.mk_adj, _ = OI._fields(self.f, self.y0)
        self.P = self.lib.gode_gcn_ode_theta_len(d)

    def call(self, export, *args):
        self.L.check(getattr(self.lib, export)(*args, self.L.stream_ptr()), export)

    def structs(self, adjoint):
        s, w = self.fwd.s, self.fwd.w
        return self.G._func_struct(s), w.workspace_struct(adjoint, s.groups)

    def forward(self, export, head, n_steps=N_STEPS):
        y = self.y0.clone()
        ky = self.fwd.w.stage_buffers(False)[0]
        fs, ws = self.structs(False)
        res = ctypes.c_void_p()
        self.call(export, *head, ctypes.byref(fs), self.L.ptr(y), ctypes.byref(res), ctypes.byref(ws), T0, T1, n_steps)
        return self.G._by_ptr(res.value, [y] + ky).clone()

    def forward_save(self, export, head, S, y_start, i0, i1):
        rec = torch.empty((i1 - i0, S + 1, self.n, self.d), device=self.dev)
        rec[0, 0].copy_(y_start)
        y_end = torch.empty_like(self.y0)
        fs, ws = self.structs(False)
        self.call(export, *head, ctypes.byref(fs), self.L.ptr(rec[0, 0]), self.L.ptr(y_end), self.L.ptr(rec), ctypes.byref(ws),
                  T0, T1, N_STEPS, i0, i1)
        return rec, y_end

    def backprop(self, export, head, rec, i0, i1):
        a, theta = self.a1.clone(), torch.zeros(self.P, device=self.dev)
        w = self.fwd.w
        ka = w.stage_buffers(True)[1]
        fs, ws = self.structs(True)
        res = ctypes.c_void_p()
        self.call(export, *head, ctypes.byref(fs), self.L.ptr(rec), self.L.ptr(a), self.L.ptr(theta), ctypes.byref(res),
                  ctypes.byref(ws), self.L.ptr(w.cot_colpart()), T0, T1, N_STEPS, i0, i1)
        return self.G._by_ptr(res.value, [a] + ka).clone(), theta

    def adjoint(self, export, head, y1):
        """-> (y, a, theta), or None where the entry point is not offered on this route (GODE_E_UNSUPPORTED)."""
        adj = self.mk_adj()
        comps = adj.new_state(y1)
        comps[1].copy_(self.a1)
        ky, ka, _, _ = adj.w.stage_buffers(True)
        fs, ws = self.G._func_struct(adj.s), adj.w.workspace_struct(True, adj.s.groups)
        yr, ar = ctypes.c_void_p(), ctypes.c_void_p()
        rc = getattr(self.lib, export)(*head, ctypes.byref(fs), self.L.ptr(comps[0]), self.L.ptr(comps[1]), self.L.ptr(adj.theta),
                                       ctypes.byref(yr), ctypes.byref(ar), ctypes.byref(ws), T1, T0, N_STEPS, self.L.stream_ptr())
        if rc == self.G.E_UNSUPPORTED:
            return None
        self.L.check(rc, export)
        return (self.G._by_ptr(yr.value, [comps[0]] + ky).clone(), self.G._by_ptr(ar.value, [comps[1]] + ka).clone(),
                adj.theta.clone())

    def stages(self, method, t, h, tol=1e-3):
        """k_1..k_S of one step from y0 (and y1, the error sums) through the one-call forward step of the method
        ("dopri5-entry": gode_gcn_ode_dopri5_step_forward)."""
        from graph_odenet_amd.solver import adaptive_stages
        S = adaptive_stages("dopri5" if method == "dopri5-entry" else method)
        kk = [[torch.zeros_like(self.y0)] for _ in range(S)]
        self.fwd.eval(t, [[(1.0, self.y0)]], kk[0])
        y1 = [torch.empty_like(self.y0)]
        if method == "dopri5-entry":
            sums = self.fwd.dopri5_step_native([self.y0], kk, y1, t, h, tol, tol)
        else:
            sums = self.fwd.adaptive_step_native(method, [self.y0], kk, y1, t, h, tol, tol)
        return [k[0] for k in kk], y1[0], sums

    def step_backprop(self, export, head, S, ks, g, kbar, wy, wk, t, h, first):
        w = self.fwd.w
        like = dict(dtype=torch.float32, device=self.dev)
        ybar = [torch.empty_like(g) for _ in range(S)]
        ybar_n, kbar1 = torch.empty_like(g), torch.zeros_like(g)
        ktheta = [torch.empty(self.P, **like) for _ in range(S)]
        theta = torch.zeros(self.P, **like)
        w.stage_buffers(True)
        fs, ws = self.structs(True)
        arr = lambda ts: (ctypes.c_void_p * S)(*[x.data_ptr() for x in ts])      # noqa: E731
        self.call(export, *head, ctypes.byref(fs), self.L.ptr(self.y0), arr(ks), self.L.ptr(g), self.L.ptr(kbar), float(wy),
                  (ctypes.c_double * S)(*[float(v) for v in wk]), float(t), float(h), int(first), arr(ybar), self.L.ptr(ybar_n),
                  self.L.ptr(kbar1), self.L.ptr(theta), arr(ktheta), ctypes.byref(ws), self.L.ptr(w.cot_colpart()))
        return [ybar_n, theta] + ([] if first else [kbar1])


def dump_gcn_fixed(rec, p, tag):
    from graph_odenet_amd.solver import method_code, n_stages
    rec(tag + ".rk4_forward.y", p.forward("gode_gcn_ode_rk4_forward", ()))
    save, y_end = p.forward_save("gode_gcn_ode_rk4_forward_save", (), 4, p.y0, 0, N_STEPS)
    rec(tag + ".rk4_forward_save.records", save)
    rec(tag + ".rk4_forward_save.y_end", y_end)
    part, part_end = p.forward_save("gode_gcn_ode_rk4_forward_save", (), 4, save[1, 0], 1, N_STEPS)
    rec(tag + ".rk4_forward_save.from_step_1.records", part)
    rec(tag + ".rk4_forward_save.from_step_1.y_end", part_end)
    for name, t in zip(("y", "a", "theta"), p.adjoint("gode_gcn_ode_rk4_adjoint", (), y_end)):
        rec(tag + ".rk4_adjoint." + name, t)
    for name, t in zip(("a", "theta"), p.backprop("gode_gcn_ode_rk4_backprop", (), save, 0, N_STEPS)):
        rec(tag + ".rk4_backprop." + name, t)
    for name, t in zip(("a", "theta"), p.backprop("gode_gcn_ode_rk4_backprop", (), part, 1, N_STEPS)):
        rec(tag + ".rk4_backprop.from_step_1." + name, t)
    for m in FIXED:
        head, S = (method_code(m),), n_stages(m)
        rec("%s.fixed_forward.%s.y" % (tag, m), p.forward("gode_gcn_ode_fixed_forward", head))
        save, y_end = p.forward_save("gode_gcn_ode_fixed_forward_save", head, S, p.y0, 0, N_STEPS)
        rec("%s.fixed_forward_save.%s.records" % (tag, m), save)
        rec("%s.fixed_forward_save.%s.y_end" % (tag, m), y_end)
        for name, t in zip(("a", "theta"), p.backprop("gode_gcn_ode_fixed_backprop", head, save, 0, N_STEPS)):
            rec("%s.fixed_backprop.%s.%s" % (tag, m, name), t)
        res = p.adjoint("gode_gcn_ode_fixed_adjoint", head, y_end)
        for name, t in zip(("y", "a", "theta"), res or ()):
            rec("%s.fixed_adjoint.%s.%s" % (tag, m, name), t)


def dump_gcn_adams(rec, p, tag):
    m, n, fwd = "explicit_adams", ADAMS_STEPS, p.fwd
    y = [p.y0.clone()]
    fwd.multistep_native(y, T0, T1, n, m)
    rec(tag + ".adams_forward.y", y[0])
    nd = p.n * p.d
    save = torch.empty(fwd.multistep_record_floats(m, n, n, nd), device=p.dev)
    save[:nd].copy_(p.y0.reshape(-1))
    y_end = torch.empty_like(p.y0)
    fwd.multistep_forward_save(m, save[:nd].view(p.n, p.d), y_end, save, T0, T1, n, 0, n)
    rec(tag + ".adams_forward_save.records", save)
    rec(tag + ".adams_forward_save.y_end", y_end)
    a, theta = p.a1.clone(), torch.zeros(p.P, device=p.dev)
    rec(tag + ".adams_backprop.a", fwd.multistep_backprop(m, save, a, theta, T0, T1, n))
    rec(tag + ".adams_backprop.theta", theta)
    adj = p.mk_adj()
    comps = adj.new_state(y_end)
    comps[1].copy_(p.a1)
    if adj.multistep_native(comps, T1, T0, n, m) is not None:          # the launch-bound route only
        for name, t in zip(("y", "a", "theta"), (comps[0], comps[1], adj.theta)):
            rec(tag + ".adams_adjoint." + name, t)


def sweep_variants(S, b, h, few):
    """(label, first, with kbar_last, wk): wk = h b, and with the entry before the last zeroed - with no kbar_last and
    b_S = 0 (FSAL) the last stage has no cotangent then, and neither has the one before it."""
    wk = [h * x for x in b]
    wz = list(wk)
    wz[S - 2] = 0.0
    allv = [("first%d.kbar%d.%s" % (f, kb, lbl), f, kb, w) for f in (0, 1) for kb in (0, 1) for lbl, w in (("wk", wk), ("wk0", wz))]
    return [allv[3], allv[4]] if few else allv


def dump_gcn_adaptive(rec, p, tag, few):
    from graph_odenet_amd.solver import ADAPTIVE_TABLEAUS, adaptive_code, adaptive_stages
    t, h = 0.25, 0.3
    g, kb = seeded((p.n, p.d), 3 * p.d).to(p.dev), seeded((p.n, p.d), 3 * p.d + 1, 0.1).to(p.dev)
    for m in ("dopri5-entry",) + ADAPTIVE:
        name = "dopri5" if m == "dopri5-entry" else m
        S, b = adaptive_stages(name), ADAPTIVE_TABLEAUS[name][2]
        ks, y1, sums = p.stages(m, t, h)
        step = "dopri5_step" if m == "dopri5-entry" else "adaptive_step"
        rec("%s.%s_forward.%s.k" % (tag, step, name), torch.stack(ks))
        rec("%s.%s_forward.%s.y1" % (tag, step, name), y1)
        rec("%s.%s_forward.%s.sums" % (tag, step, name), sums)
        export, head = ("gode_gcn_ode_dopri5_step_backprop", ()) if m == "dopri5-entry" else \
            ("gode_gcn_ode_adaptive_step_backprop", (adaptive_code(name),))
        for label, first, with_kb, wk in sweep_variants(S, b, h, few):
            out = p.step_backprop(export, head, S, ks, g, kb if with_kb else None, 0.9, wk, t, h, first)
            for nm, x in zip(("ybar_n", "theta", "kbar1"), out):
                rec("%s.%s_backprop.%s.%s.%s" % (tag, step, name, label, nm), x)


# ---- GAT ------------------------------------------------------------------------------------------------------------------
class Gat:
    def __init__(self, n, d, H, E, dev):
        from graph_odenet_amd import _lib, gat_heads, gat_models, gat_ode
        gat_ode.GatOdeField.ADAPTIVE_NATIVE = True
        self.L, self.lib, self.dev, self.n, self.d = _lib, _lib.load(), dev, n, d
        gen = torch.Generator().manual_seed(17)
        src = torch.cat([torch.randint(0, n, (E - n,), generator=gen), torch.arange(n)])
        tgt = torch.cat([torch.randint(0, n, (E - n,), generator=gen), torch.arange(n)])
        mt = torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(E)]), torch.ones(E), (n, E))
        torch.manual_seed(5)
        f = gat_models.ODEfunc(d) if H == 1 else gat_heads.ODEfunc(d, H)
        with torch.no_grad():
            f.norm1.weight.add_(0.3 * torch.randn(d))
            f.norm1.bias.add_(0.3 * torch.randn(d))
        self.f = f.to(dev)
        self.f.set_adj(src.to(dev), tgt.to(dev), mt.to(dev))
        x = 0.5 * seeded((n, d), 9)
        if d == 64:      # two channels per GroupNorm group: keep each pair apart (tests/test_gpu_gat_backprop.py: x0_of)
            s = 3.0 * (2.0 * torch.randint(0, 2, (n, d // 2), generator=torch.Generator().manual_seed(10)) - 1.0)
            x[:, 0::2] += s
            x[:, 1::2] -= s
        self.y0, self.a1 = x.to(dev), seeded((n, d), 11).to(dev)
        self.fwd, self.mk_adj, _ = self.f.gode_fields(self.y0)
        self.fwd.prepare()
        assert self.fwd.small() and self.fwd.rk4_backprop is not None, "the launch-bound route"
        assert self.fwd.raw_logits() == (H > 1 and E * H > 8192), "raw-logit route"

    def call(self, export, *args):
        self.L.check(getattr(self.lib, export)(*args, self.L.stream_ptr()), export)

    def forward_save(self, export, head, S):
        rec = torch.empty((N_STEPS, S + 1, self.n, self.d), device=self.dev)
        rec[0, 0].copy_(self.y0)
        y_end = torch.empty_like(self.y0)
        fs, ws = self.fwd._structs(True)
        self.call(export, *head, ctypes.byref(fs), self.L.ptr(rec[0, 0]), self.L.ptr(y_end), self.L.ptr(rec), ctypes.byref(ws),
                  T0, T1, N_STEPS, 0, N_STEPS)
        return rec, y_end

    def backprop(self, export, head, S, rec):
        a, theta = self.a1.clone(), self.fwd.packed_grads(self.dev)
        fs, ws = self.fwd._structs(True)
        sw = self.fwd._sweep_work()
        ybar = (ctypes.c_void_p * S)(*[b.data_ptr() for b in sw.ybar[:S]])
        self.call(export, *head, ctypes.byref(fs), self.L.ptr(rec), self.L.ptr(a), self.L.ptr(theta), ybar, self.L.ptr(sw.k_scratch),
                  self.L.ptr(sw.parts), ctypes.byref(ws), T0, T1, N_STEPS, 0, N_STEPS)
        return a, theta

    def stages(self, method, t, h, tol=1e-3):
        from graph_odenet_amd.solver import adaptive_stages
        S = adaptive_stages(method)
        kk = [[torch.zeros_like(self.y0)] for _ in range(S)]
        self.fwd.eval(t, [[(1.0, self.y0)]], kk[0])
        y1 = [torch.empty_like(self.y0)]
        self.fwd.adaptive_step_native(method, [self.y0], kk, y1, t, h, tol, tol)
        return [k[0] for k in kk]

    def step_backprop(self, export, head, S, ks, g, kbar, wy, wk, t, h, first):
        fs, ws = self.fwd._structs(True)
        sw = self.fwd._sweep_work()
        ybar_n, kbar1 = sw.pairs[0]
        kbar1.zero_()
        theta = self.fwd.packed_grads(self.dev)
        kptr = (ctypes.c_void_p * S)(*[x.data_ptr() for x in ks])
        ybar = (ctypes.c_void_p * S)(*[b.data_ptr() for b in sw.ybar[:S]])
        self.call(export, *head, ctypes.byref(fs), self.L.ptr(self.y0), kptr, self.L.ptr(g), self.L.ptr(kbar), float(wy),
                  (ctypes.c_double * S)(*[float(v) for v in wk]), float(t), float(h), int(first), ybar, self.L.ptr(ybar_n),
                  self.L.ptr(kbar1), self.L.ptr(theta), self.L.ptr(sw.k_scratch), self.L.ptr(sw.parts), ctypes.byref(ws))
        return [ybar_n, theta] + ([] if first else [kbar1])


def dump_gat(rec, p, tag):
    from graph_odenet_amd.solver import ADAPTIVE_TABLEAUS, adaptive_code, adaptive_stages, method_code, n_stages
    for export, head, S, name in [("rk4", (), 4, "rk4_entry")] + [("fixed", (method_code(m),), n_stages(m), m) for m in FIXED]:
        save, y_end = p.forward_save("gode_gat_ode_%s_forward_save" % export, head, S)
        rec("%s.%s_forward_save.%s.records" % (tag, export, name), save)
        rec("%s.%s_forward_save.%s.y_end" % (tag, export, name), y_end)
        for nm, x in zip(("a", "theta"), p.backprop("gode_gat_ode_%s_backprop" % export, head, S, save)):
            rec("%s.%s_backprop.%s.%s" % (tag, export, name, nm), x)
    t, h = 0.25, 0.3
    g, kb = seeded((p.n, p.d), 21).to(p.dev), seeded((p.n, p.d), 22, 0.1).to(p.dev)
    for m in ("dopri5-entry",) + ADAPTIVE:
        name = "dopri5" if m == "dopri5-entry" else m
        S, b = adaptive_stages(name), ADAPTIVE_TABLEAUS[name][2]
        ks = p.stages(name, t, h)
        export, head = ("gode_gat_ode_dopri5_step_backprop", ()) if m == "dopri5-entry" else \
            ("gode_gat_ode_adaptive_step_backprop", (adaptive_code(name),))
        step = "dopri5_step" if m == "dopri5-entry" else "adaptive_step"
        for label, first, with_kb, wk in sweep_variants(S, b, h, False):
            out = p.step_backprop(export, head, S, ks, g, kb if with_kb else None, 0.9, wk, t, h, first)
            for nm, x in zip(("ybar_n", "theta", "kbar1"), out):
                rec("%s.%s_backprop.%s.%s.%s" % (tag, step, name, label, nm), x)


SECTIONS = ("gcn-small", "gcn-multi", "gcn-large128", "gcn-large64", "gat")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--against", default=None)
    ap.add_argument("--list", default=None, help="with --against: also write the list of compared arrays here")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--sections", default=",".join(SECTIONS))
    args = ap.parse_args()
    assert bool(args.out) != bool(args.against), "one of --out, --against"
    sys.path.insert(0, os.path.abspath(args.root))
    from graph_odenet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    rec = Recorder(args.out, args.against)
    sections = args.sections.split(",")
    with torch.no_grad():
        if "gcn-small" in sections or "gcn-multi" in sections:
            g = uniform_graph(300, dev)
            for tag, fused in (("gcn-small", 1), ("gcn-multi", 0)):
                if tag not in sections:
                    continue
                old = lib.gode_get_option(b"small_fused")
                assert lib.gode_set_option(b"small_fused", fused) == 0
                p = Gcn(g, 16, dev)
                dump_gcn_fixed(rec, p, tag)
                dump_gcn_adams(rec, p, tag)
                dump_gcn_adaptive(rec, p, tag, few=False)
                lib.gode_set_option(b"small_fused", old)
                del p
        if "gcn-large128" in sections or "gcn-large64" in sections:
            g = uniform_graph(65_600, dev)
            if "gcn-large128" in sections:
                p = Gcn(g, 128, dev)
                dump_gcn_fixed(rec, p, "gcn-large128")
                del p
                torch.cuda.empty_cache()
            if "gcn-large64" in sections:
                p = Gcn(g, 64, dev)
                dump_gcn_fixed(rec, p, "gcn-large64")
                dump_gcn_adams(rec, p, "gcn-large64")
                dump_gcn_adaptive(rec, p, "gcn-large64", few=True)
                del p
        if "gat" in sections:
            for tag, d, H, E in (("gat-1x16", 16, 1, 1400), ("gat-8x8-E900", 64, 8, 900), ("gat-8x8-E1400", 64, 8, 1400)):
                dump_gat(rec, Gat(600, d, H, E, dev), tag)
    torch.cuda.synchronize()
    summary = "%d arrays %s%s" % (len(rec.lines), "compared" if args.against else "written",
                                  ", %d differ" % rec.bad if args.against else "")
    print(summary)
    if args.list:
        with open(args.list, "w") as fh:
            fh.write("\n".join(rec.lines + [summary]) + "\n")
    sys.exit(1 if rec.bad else 0)


if __name__ == "__main__":
    main()
