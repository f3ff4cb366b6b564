"""Fused GAT ODE function  f(t, x) = relu(EdgeAttention([t | GroupNorm(x)]))  (reference: GAT/models.py:172-179 ->
GAT/layers.py:95-122) and its vector-Jacobian product as plain kernel sequences over the C ABI - no autograd
graph, no per-edge E x 2i tensor.

The two Linear layers of the reference act on h_e = [x[src_e] | x[tgt_e]] (f: o x 2i, w: 1 x 2i, i = d+1 with the
time column first).  They are applied at NODE level and split by role, so that the two d x d blocks run on the square
MFMA kernels and only the two logit columns take the generic path:

  Ps = [t|xn] Wsrc   (Wsrc = Wf[:, :i]^T, i x o)      As = [t|xn] ww[:, :i]^T     z_e = Ps[src_e] + Pt[tgt_e] + bf
  Pt = [t|xn] Wtgt   (Wtgt = Wf[:, i:]^T, i x o)      At = [t|xn] ww[:, i:]^T     a_e = As[src_e] + At[tgt_e] + bw

  forward : 3 x gode_gn_time_gemm_f32 (GroupNorm + time column fused; a multi-term stage input is combined once and
            written out by the first launch), gode_gat_logits_f32, gode_gat_agg_f32_fwd (a message activation other than
            relu: its gode_gat_act_t with outer_relu, so that it applies the function's outer relu as well)
  adjoint : + gode_gat_agg_f32_bwd (stage cotangent combined and relu-masked inside), gode_gat_maxpath_f32,
            gode_gat_scatter_f32 (all four incidence sums in one launch), 3 x gode_gn_time_gemm_bwd_f32 (accumulating
            into k_a), 3 x gode_wgrad_f32 + reductions, gode_time_row_fixup_f32, column sums for the biases.

H heads (gat_heads.py) run the same sequence on the H-fold graph, with d = H * o: Wlog has 2H columns, bw H entries, the
message biases bf are folded into Pt and the logits are shifted by their head's maximum (gode_gat_logits_heads_f32),
so that the aggregation runs with zero bias and amax = 0.  The branches on H are those of csrc/gat_driver.hip.

The adjoint integrates [y, a, a_t, theta] with theta = [Wsrc | Wtgt | Wlog | bf | bw | gamma | beta] packed in ONE
buffer (one RK combine launch for all parameters); the gradient is converted back to the parameters' layout once,
at the end of the solve.

Backprop through the solve (odeint, adjoint=False) on launch-bound graphs - GatOdeField.small(), no padded logit columns:
the forward field offers the backprop half of solver.Field's protocol, issued from C (csrc/gat_driver.hip:
gode_gat_ode_rk4_forward_save / _rk4_backprop / _dopri5_step_backprop, and - with GatOdeField.ADAPTIVE_NATIVE on -
gode_gat_ode_adaptive_step_backprop for bosh3 and adaptive_heun).  The reverse of a stage is the adjoint stage's
launch sequence with the stage's cotangent kbar_s in place of -a; each swept stage leaves its parameter partials in a slot of
its own and one gode_gat_small_close_stages_f32 launch per step adds them to the packed theta.  Elsewhere the members stay
None and odeint re-runs each interval as torch ops under autograd.
"""
import ctypes
import os

import torch

from . import _lib, ops
from .gat_layers import message_activation
from .solver import Field, adaptive_code, adaptive_stages, method_code


# launch-bound graphs: the reduction launches that close an adjoint stage run as one (ops.reduce_segments_); larger graphs
# keep the separate launches (the weight-gradient reduction has a 16-byte form that matters there)
MERGED_FINISH_MAX_ROWS = 1 << 16
# H heads on at least this many nodes: the 2H logit columns ride the square MFMA kernels as a zero-padded (d+1) x d block
# (0.4-0.5 ms per product at 2^20 x 128 against 2.2 / 5.5 / 3.8 ms for the generic kernels on a (d+1) x 16 block);
# smaller graphs are launch-bound and keep the compact product
PAD_LOGITS_MIN_ROWS = 4096


class GatOdeSpec:
    """Packed description of relu(layer([t | norm(x)])) on n nodes: theta = [Wsrc | Wtgt | Wlog | bf | bw | gamma | beta]
    with Wsrc, Wtgt (d+1) x d (head h in columns h*o..), Wlog (d+1) x 2H, bf d, bw H.  eg is the graph the kernels see
    (the H-fold graph with H > 1 heads); layer is the reference's layer, or a MultiHeadGraphConvolution."""

    def __init__(self, eg, n, layer, norm, act_layer=None):
        self.eg, self.n, self.layer, self.norm = eg, n, layer, norm
        self.heads = H = getattr(layer, "n_heads", 1)
        self.d, self.i = d, i = layer.out_features, layer.in_features
        if i != d + 1:
            raise ValueError("GatOdeSpec: the ODE layer maps d+1 -> d features")
        self.o = d // H
        self.groups, self.eps_gn, self.eps = int(norm.num_groups), float(norm.eps), float(layer.eps)
        self.act = message_activation(layer.act if act_layer is None else act_layer.act)       # (code, param); None: no kernel form
        f = dict(dtype=torch.float32, device=norm.weight.device)
        self.Wsrc, self.Wtgt, self.Wlog = torch.empty(i, d, **f), torch.empty(i, d, **f), torch.empty(i, 2 * H, **f)
        self.pad_logits = n >= PAD_LOGITS_MIN_ROWS and d in (16, 32, 64, 128) and 4 < 2 * H <= d
        self.Wlog_pad = torch.zeros(i, d, **f) if self.pad_logits else None
        self.Wpacked = None                           # LDS images of the three blocks for the one-launch kernels (d >= 32)
        if H == 1:
            self.bf, self.bw = layer.f.bias.detach(), layer.w.bias.detach()
        else:
            self.bf, self.bw = torch.empty(d, **f), torch.empty(H, **f)
        self.gamma, self.beta = norm.weight.detach(), norm.bias.detach()
        self.refresh()
        # offsets inside the packed parameter-gradient buffer
        self.off, p = {}, 0
        for name, ln in (("Wsrc", i * d), ("Wtgt", i * d), ("Wlog", i * 2 * H), ("bf", d), ("bw", H), ("gamma", d), ("beta", d)):
            self.off[name] = (p, p + ln)
            p += ln
        self.n_theta = p

    def refresh(self):
        """Re-pack the weights by role, in place (at the start of every solve: the parameters move between solves, the
        buffers - and a HIP graph captured over them - do not)."""
        if self.heads == 1:
            Wf, ww = self.layer.f.weight.detach(), self.layer.w.weight.detach()
            i = self.i
            self.Wsrc.copy_(Wf[:, :i].t())
            self.Wtgt.copy_(Wf[:, i:].t())
            self.Wlog[:, 0].copy_(ww[0, :i])
            self.Wlog[:, 1].copy_(ww[0, i:])
        else:
            with torch.no_grad():
                Wsrc, Wtgt, Wlog, bf, ba = self.layer.packed()
                self.Wsrc.copy_(Wsrc); self.Wtgt.copy_(Wtgt); self.Wlog.copy_(Wlog); self.bf.copy_(bf); self.bw.copy_(ba[1::2])
                if self.pad_logits:
                    self.Wlog_pad[:, :2 * self.heads].copy_(Wlog)
        # Wpacked (csrc/gat_small.hip: gode_gat_small_pack_f32) follows the weights.  Worth a launch per solve from d = 32
        # on (at d = 16 the blocks are 2.4 KB and the kernels lay them out themselves).
        if not self.pad_logits and self.d >= 32 and self.Wsrc.is_cuda and \
                _lib.load().gode_gat_small_supported(self.n, self.d, self.groups, self.heads):
            self.Wpacked = ops.gat_small_pack(self.Wsrc, self.Wtgt, self.Wlog, self.heads, out=self.Wpacked)

    def views(self, theta):
        v = {k: theta[a:b] for k, (a, b) in self.off.items()}
        v["Wsrc"], v["Wtgt"] = v["Wsrc"].view(self.i, self.d), v["Wtgt"].view(self.i, self.d)
        v["Wlog"] = v["Wlog"].view(self.i, 2 * self.heads)
        return v


class _Work:
    """Buffers of one (graph, d, H): allocated once, so that neither the eager path nor a captured graph allocates."""

    def __init__(self, spec, device):
        n, d, o, H, E = spec.n, spec.d, spec.o, spec.heads, spec.eg.E
        nv = n * H
        lib = _lib.load()
        f = dict(dtype=torch.float32, device=device)
        u8 = dict(dtype=torch.uint8, device=device)
        self.X = torch.empty(n, d, **f)
        self.Ps, self.Pt, self.A2 = torch.empty(n, d, **f), torch.empty(n, d, **f), torch.empty(n, 2 * H, **f)
        self.dPs, self.dPt, self.dA2 = torch.empty(n, d, **f), torch.empty(n, d, **f), torch.empty(n, 2 * H, **f)
        self.a = torch.empty(max(E, 1), **f)[:E]
        self.wgt, self.den = torch.zeros(max(E, 1), **f)[:E], torch.empty(nv, **f)
        self.dz, self.da = torch.zeros(max(E, 1), o, **f)[:E], torch.zeros(max(E, 1), **f)[:E]
        # with H heads the n x (H*o) projections ARE the (n*H) x o projections of the virtual nodes
        self.proj = ops.gat_proj(self.Ps.view(nv, o), self.Pt.view(nv, o), self.A2.view(nv, 2))
        self.np_b = lib.gode_gemm_bwd_parts(n)
        self.gp, self.bp = torch.empty(3 * self.np_b, d, **f), torch.empty(3 * self.np_b, d, **f)
        npw = lib.gode_wgrad_parts(n)
        nl = spec.i * (d if spec.pad_logits else 2 * H)
        self.wp = [torch.empty(npw, spec.i * d, **f), torch.empty(npw, spec.i * d, **f), torch.empty(npw, nl, **f)]
        if H == 1:
            self.amax = torch.empty(1, **f)
            self.logits_scratch = torch.empty(max(lib.gode_gat_logits_scratch_bytes(E), 16), **u8)
        else:
            # zero message bias and maximum of the edge kernels (the biases ride Pt and the logits kernel)
            self.zero, self.bf0, self.zeros = torch.zeros(1, **f), torch.zeros(o, **f), torch.zeros(max(o, 1), **f)
            self.heads_scratch = torch.empty(max(lib.gode_gat_heads_scratch_bytes(E, H), 16), **u8)
            self.ba_grad = torch.empty(2 * H, **f)
        if spec.pad_logits:
            self.A2pad, self.dA2pad = torch.empty(n, d, **f), torch.zeros(n, d, **f)     # columns >= 2H of dA2pad stay 0
            self.gWlog_pad = torch.empty(spec.i, d, **f)
        # extras of the C-level dopri5 step (csrc/gat_driver.hip)
        self.pair = torch.empty(2 * H, **f)
        self.colsum_scratch = torch.empty(max(lib.gode_colsum_scratch_bytes(n, d), 16), **u8)
        self.colsum_scratch2 = torch.empty(max(lib.gode_colsum_scratch_bytes(n, 2 * H), 16), **u8)
        # the dopri5 drivers' error norm and the tableau-driven drivers' fused close share it: the larger of the two
        self.err_scratch = torch.empty(max(lib.gode_rk_errnorm_scratch_bytes(), lib.gode_rk_close_err_scratch_bytes()), **u8)
        # launch-bound graphs: block partials of the one-launch dense VJP (csrc/gat_small.hip)
        small = not spec.pad_logits and lib.gode_gat_small_supported(n, d, spec.groups, H)
        self.small_part = ops.gat_small_part(n, d, H, device) if small else None
        self.step_parts = None                 # four such buffers, one per stage of a fixed-grid step (allocated on first use)
        self.sweep = None                      # work arrays of the backprop sweeps (_SweepWork, allocated on first use)
        self.adj_parts = None                  # partial slots of a one-call adaptive adjoint step (allocated on first use)


class _SweepWork:
    """Work arrays of the backprop sweeps of one (graph, d, H): 7 Ybar (rk4 uses four), two (ybar_n, kbar_1) pairs that take
    turns from step to step, the re-evaluated stage derivative and 7 slots of parameter partials."""

    def __init__(self, spec, small_part):
        f = dict(dtype=torch.float32, device=small_part.device)
        self.ybar = [torch.empty(spec.n, spec.d, **f) for _ in range(7)]
        self.pairs = [(torch.empty(spec.n, spec.d, **f), torch.empty(spec.n, spec.d, **f)) for _ in range(2)]
        self.k_scratch = torch.empty(spec.n, spec.d, **f)
        self.parts = torch.empty(7 * small_part.numel(), **f)


def theta_param_grads(s, order, theta):
    """The packed gradient theta (laid out as GatOdeSpec.off) in the parameters' own layout, in `order` (the names
    gat_fields gives func.parameters()): one head or H."""
    i, o, H = s.i, s.o, s.heads
    if H == 1:
        v = s.views(theta)
        gWf = torch.cat([v["Wsrc"].t(), v["Wtgt"].t()], 1).contiguous()                          # o x 2i
        gww = torch.cat([v["Wlog"][:, 0], v["Wlog"][:, 1]]).view(1, 2 * i).contiguous()           # 1 x 2i
        m = {"gamma": v["gamma"].clone(), "beta": v["beta"].clone(), "Wf": gWf, "bf": v["bf"].clone(),
             "ww": gww, "bw": v["bw"].clone()}
        return [m[k] for k in order]
    v = s.views(theta.clone())                       # one copy; everything below is a view of it or one permuted copy
    m = {"gamma": v["gamma"], "beta": v["beta"]}
    gWf = torch.cat([v["Wsrc"].view(i, H, o).permute(1, 2, 0), v["Wtgt"].view(i, H, o).permute(1, 2, 0)], 2)    # H x o x 2i
    gww = v["Wlog"].view(i, H, 2).permute(1, 2, 0).reshape(H, 1, 2 * i)                                         # H x 1 x 2i
    gbf, gbw = v["bf"].view(H, o), v["bw"].view(H, 1)
    for h in range(H):
        m["Wf%d" % h], m["bf%d" % h], m["ww%d" % h], m["bw%d" % h] = gWf[h], gbf[h], gww[h], gbw[h]
    return [m[k] for k in order]


class GatOdeField(Field):
    """f(t, x) = relu(layer([t | GroupNorm(x)])) as a kernel sequence.  Adaptive steps run as one C call
    (csrc/gat_driver.hip) except with padded logit columns (H heads above PAD_LOGITS_MIN_ROWS nodes), where the solver
    takes the per-stage path.  Built with the parameter order (gat_fields) on a launch-bound graph - small(), no padded
    logit columns - it also offers the backprop half of the protocol (solver.Field), issued from csrc/gat_driver.hip."""
    n_components = 1
    fused = True
    BACKPROP_FUSED = True            # False: no backprop members (odeint re-runs each interval as torch ops under autograd)
    # bosh3 / adaptive_heun on the one-call step and the fused sweep (csrc/gat_driver.hip: gode_gat_ode_adaptive_step_*).  An
    # opt-in (the environment's GODE_GAT_ADAPTIVE_NATIVE=1, or this attribute set before the fields are built): off, the fields
    # offer no adaptive_* member and the two methods run on the per-stage driver as before (generic backprop under
    # adjoint=False) - what tests/test_gpu_adaptive_methods.py: test_gat_bosh3 states of a GAT field
    ADAPTIVE_NATIVE = os.environ.get("GODE_GAT_ADAPTIVE_NATIVE", "0") == "1"

    def __init__(self, spec, work, order=None):
        self.s, self.w = spec, work
        self.token = ("gat-heads" if spec.heads > 1 else "gat", id(spec.eg))
        if spec.pad_logits:
            self.dopri5_step_native = None
        elif self.ADAPTIVE_NATIVE:
            self.adaptive_step_native = self._adaptive_step_native      # a member of the instance, as the sweeps below
        if order is not None and self.BACKPROP_FUSED and not spec.pad_logits and self.small():
            self.order = order
            self.rk4_forward_save, self.rk4_backprop = self._rk4_forward_save, self._rk4_backprop
            self.fixed_forward_save, self.fixed_backprop = self._fixed_forward_save, self._fixed_backprop
            self.dopri5_step_backprop, self.dopri5_backprop_work = self._dopri5_step_backprop, self._dopri5_backprop_work
            if self.ADAPTIVE_NATIVE:
                self.adaptive_step_backprop, self.adaptive_backprop_work = self._adaptive_step_backprop, self._adaptive_backprop_work
            self.packed_grads, self.packed_param_grads = self._packed_grads, self._packed_param_grads

    def prepare(self):
        self.s.refresh()

    def small(self):
        """The dense half runs on the one-launch kernels of csrc/gat_small.hip (launch-bound graphs; option small_fused)."""
        return self.w.small_part is not None and ops.gat_small_supported(self.s.n, self.s.d, self.s.groups, self.s.heads)

    def raw_logits(self):
        """H heads on launch-bound graphs: no launch that shifts the logits - the aggregation reduces its head's partial
        maxima."""
        s = self.s
        return s.heads > 1 and s.n * s.heads <= 65536 and s.eg.E > 8192 and self.small()

    # ---- one adaptive step per C call (csrc/gat_driver.hip) -------------------------------------------------------
    def _structs(self, adjoint):
        s, w, eg = self.s, self.w, self.s.eg
        fs = _lib.GatOdeFunc()
        fs.mt = ops._edge_csr(eg, s.o + 4)
        for name, gph in (("ms_inc", eg.Ms_inc), ("mt_inc", eg.Mt_inc)):
            gs = _lib.Graph()
            gs.rowptr, gs.col, gs.val = gph.rowptr.data_ptr(), gph.col.data_ptr(), None
            gs.items, gs.n_items = (gph.items.data_ptr() if gph.items is not None else None), gph.n_items
            gs.long_rows = gph.long_rows.data_ptr() if gph.long_rows is not None else None
            gs.n_long = gph.n_long
            part = gph.partial(s.o) if adjoint else None
            gs.partial = part.data_ptr() if part is not None else None
            gs.n_rows, gs.nnz = gph.n_rows, gph.nnz
            setattr(fs, name, gs)
        p = lambda t: (t.data_ptr() or None) if t is not None else None      # noqa: E731  (struct fields take ints)
        fs.src, fs.tgt, fs.n_edges = p(eg.src), p(eg.tgt), eg.E
        fs.n, fs.d, fs.groups, fs.eps_gn, fs.eps = s.n, s.d, s.groups, s.eps_gn, s.eps
        fs.Wsrc, fs.Wtgt, fs.Wlog = s.Wsrc.data_ptr(), s.Wtgt.data_ptr(), s.Wlog.data_ptr()
        fs.bf, fs.bw, fs.gamma, fs.beta = s.bf.data_ptr(), s.bw.data_ptr(), s.gamma.data_ptr(), s.beta.data_ptr()
        fs.Wpacked = s.Wpacked.data_ptr() if s.Wpacked is not None else None
        fs.act, fs.act_param = int(s.act[0]), float(s.act[1])
        ws = _lib.GatWorkspace()
        for k in ("X", "Ps", "Pt", "A2", "a", "wgt", "den"):
            setattr(ws, k, p(getattr(w, k)))
        if s.heads > 1:
            fs.heads = s.heads
            ws.zeros, ws.heads_scratch = p(w.zeros), p(w.heads_scratch)
            ws.amax, ws.logits_scratch = p(w.zero), p(w.heads_scratch)          # unused by the heads sequence, must be set
        else:
            ws.amax, ws.logits_scratch = p(w.amax), p(w.logits_scratch)
        if adjoint:
            for k in ("dz", "da", "dPs", "dPt", "dA2", "pair", "gp", "bp", "colsum_scratch", "colsum_scratch2"):
                setattr(ws, k, p(getattr(w, k)))
            for j in range(3):
                ws.wp[j] = w.wp[j].data_ptr()
            ws.maxpath_scratch = p(w.heads_scratch if s.heads > 1 else eg.maxpath_scratch())
            ws.small_part = p(w.small_part)
        return fs, ws

    def dopri5_step_native(self, y, kk, y1, t, h, rtol, atol):
        lib = _lib.load()
        fs, ws = self._structs(False)
        kptr = (ctypes.c_void_p * 7)(*[kk[i][0].data_ptr() for i in range(7)])
        sums = torch.empty(1, dtype=torch.float64, device=y[0].device)
        _lib.check(lib.gode_gat_ode_dopri5_step_forward(ctypes.byref(fs), _lib.ptr(y[0]), kptr, _lib.ptr(y1[0]), ctypes.byref(ws),
                                                        float(t), float(h), float(rtol), float(atol), _lib.ptr(sums),
                                                        _lib.ptr(self.w.err_scratch), _lib.stream_ptr()),
                   "gode_gat_ode_dopri5_step_forward")
        return sums

    def _adaptive_step_native(self, method, y, kk, y1, t, h, rtol, atol):
        """dopri5_step_native for any adaptive method (kk: S stage buffers): gode_gat_ode_adaptive_step_forward, which closes
        the step with the fused launch (solution and error sum from one pass over the stages)."""
        lib = _lib.load()
        S = adaptive_stages(method)
        fs, ws = self._structs(False)
        kptr = (ctypes.c_void_p * S)(*[kk[i][0].data_ptr() for i in range(S)])
        sums = torch.empty(1, dtype=torch.float64, device=y[0].device)
        _lib.check(lib.gode_gat_ode_adaptive_step_forward(adaptive_code(method), ctypes.byref(fs), _lib.ptr(y[0]), kptr,
                                                          _lib.ptr(y1[0]), ctypes.byref(ws), float(t), float(h), float(rtol),
                                                          float(atol), _lib.ptr(sums), _lib.ptr(self.w.err_scratch),
                                                          _lib.stream_ptr()),
                   "gode_gat_ode_adaptive_step_forward")
        return sums

    # ---- backprop through the solve (odeint._OdeintBackprop): launch-bound graphs, csrc/gat_driver.hip ------------------
    def _packed_grads(self, device):
        """Zeroed theta = [Wsrc | Wtgt | Wlog | bf | bw | gamma | beta]."""
        return torch.zeros(self.s.n_theta, dtype=torch.float32, device=device)

    def _packed_param_grads(self, theta):
        return theta_param_grads(self.s, self.order, theta)

    def _sweep_work(self):
        w = self.w
        if w.sweep is None:
            w.sweep = _SweepWork(self.s, w.small_part)
        return w.sweep

    def _rk4_forward_save(self, y0, y_end, save, t0, t1, n_steps, i0, i1):
        self._fixed_forward_save("rk4", y0, y_end, save, t0, t1, n_steps, i0, i1)

    def _rk4_backprop(self, save, a, theta, t0, t1, n_steps, i0, i1):
        return self._fixed_backprop("rk4", save, a, theta, t0, t1, n_steps, i0, i1)

    def _fixed_forward_save(self, method, y0, y_end, save, t0, t1, n_steps, i0, i1):
        """Steps i0 .. i1-1 with the launches of solver.integrate_fixed on this field (the same bits; rk4: integrate_rk4's);
        save[r] = [y_n, k_1..k_S] of step i0 + r."""
        fs, ws = self._structs(True)
        _lib.check(_lib.load().gode_gat_ode_fixed_forward_save(
            method_code(method), ctypes.byref(fs), _lib.ptr(y0), _lib.ptr(y_end), _lib.ptr(save), ctypes.byref(ws), float(t0),
            float(t1), int(n_steps), int(i0), int(i1), _lib.stream_ptr()), "gode_gat_ode_fixed_forward_save")

    def _fixed_backprop(self, method, save, a, theta, t0, t1, n_steps, i0, i1):
        """Reverse sweep over the records of steps i0 .. i1-1 (_fixed_forward_save); `a` is advanced in place and returned,
        theta incremented."""
        fs, ws = self._structs(True)
        sw = self._sweep_work()
        ybar = (ctypes.c_void_p * 4)(*[b.data_ptr() for b in sw.ybar[:4]])
        _lib.check(_lib.load().gode_gat_ode_fixed_backprop(
            method_code(method), ctypes.byref(fs), _lib.ptr(save), _lib.ptr(a), _lib.ptr(theta), ybar, _lib.ptr(sw.k_scratch),
            _lib.ptr(sw.parts), ctypes.byref(ws), float(t0), float(t1), int(n_steps), int(i0), int(i1), _lib.stream_ptr()),
            "gode_gat_ode_fixed_backprop")
        return a

    def _dopri5_backprop_work(self, like):
        sw = self._sweep_work()
        return {"ybar": sw.ybar, "pairs": sw.pairs}

    def _step_backprop(self, export, head, S, y, k, g, kbar_last, wy, wk, t, h, first, work, turn, theta):
        """Reverse sweep over one accepted step of an S-stage adaptive method (k, wk of S entries; kbar_last arrives on k_S)
        through `export`, whose leading arguments are `head`.  Returns (ybar_n, kbar_1) in work["pairs"][turn]; kbar_1 is None
        when `first`."""
        fs, ws = self._structs(True)
        sw = self._sweep_work()
        ybar_n, kbar1 = work["pairs"][turn]
        kptr = (ctypes.c_void_p * S)(*[x.data_ptr() for x in k])
        ybar = (ctypes.c_void_p * S)(*[b.data_ptr() for b in work["ybar"][:S]])
        wka = (ctypes.c_double * S)(*[float(v) for v in wk])
        _lib.check(getattr(_lib.load(), export)(
            *head, ctypes.byref(fs), _lib.ptr(y), kptr, _lib.ptr(g), _lib.ptr(kbar_last), float(wy), wka, float(t), float(h),
            1 if first else 0, ybar, _lib.ptr(ybar_n), _lib.ptr(kbar1), _lib.ptr(theta), _lib.ptr(sw.k_scratch),
            _lib.ptr(sw.parts), ctypes.byref(ws), _lib.stream_ptr()), export)
        return ybar_n, (None if first else kbar1)

    def _dopri5_step_backprop(self, y, k, g, kbar7, wy, wk, t, h, first, work, turn, theta):
        """The sweep under dopri5 through its own entry point (same body in C): the member is offered with ADAPTIVE_NATIVE off
        as well, and a refusal names gode_gat_ode_dopri5_step_backprop."""
        return self._step_backprop("gode_gat_ode_dopri5_step_backprop", (), 7, y, k, g, kbar7, wy, wk, t, h, first, work, turn,
                                   theta)

    def _adaptive_backprop_work(self, method, like):
        """_dopri5_backprop_work for any adaptive method: _SweepWork's 7 Ybar and 7 slots serve every S."""
        return self._dopri5_backprop_work(like)

    def _adaptive_step_backprop(self, method, y, k, g, kbar_last, wy, wk, t, h, first, work, turn, theta):
        """The sweep under any adaptive method (k, wk of S entries): gode_gat_ode_adaptive_step_backprop."""
        return self._step_backprop("gode_gat_ode_adaptive_step_backprop", (adaptive_code(method),), adaptive_stages(method), y, k,
                                   g, kbar_last, wy, wk, t, h, first, work, turn, theta)

    def _project(self, t, y_terms):
        """Ps, Pt, A2 of the stage input; returns the term list later launches of the stage should read."""
        s, w = self.s, self.w
        x_out = w.X if len(y_terms) > 1 else None
        terms = [(1.0, w.X)] if x_out is not None else y_terms
        if self.small():
            ops.gat_project_small(y_terms, s.n, s.d, s.groups, s.eps_gn, s.gamma, s.beta, s.Wsrc, s.Wtgt, s.Wlog, s.heads,
                                  s.bf if s.heads > 1 else None, t, w.Ps, w.Pt, w.A2, x_out=x_out, packed=s.Wpacked)
            return terms
        ops.gn_time_gemm_pair(y_terms, s.n, s.d, s.groups, s.eps_gn, s.gamma, s.beta, s.Wsrc, s.Wtgt, True, t, w.Ps, w.Pt,
                              x_out=x_out)
        if s.pad_logits:
            ops.gn_time_gemm(terms, s.n, s.d, s.groups, s.eps_gn, s.gamma, s.beta, s.Wlog_pad, True, t, out=w.A2pad)
            w.A2.copy_(w.A2pad[:, :2 * s.heads])
        else:
            ops.gn_time_gemm(terms, s.n, s.d, s.groups, s.eps_gn, s.gamma, s.beta, s.Wlog, True, t, out=w.A2)
        if s.heads > 1:
            w.Pt.add_(s.bf)                              # per-head message biases, folded into the target-side part
        return terms

    def _forward(self, t, y_terms, out):
        s, w, eg = self.s, self.w, self.s.eg
        terms = self._project(t, y_terms)
        # The outer relu of ODEfunc is the identity on a weighted mean of relu's: relu messages pass no gode_gat_act_t.
        # Under any other message activation the aggregation applies it where it stores `out` (outer_relu; csrc/gat_driver.hip:
        # eval_forward sets it under every activation, which runs the same kernels).
        act, ode = self._kernel_act()
        if s.heads == 1:
            ops.gat_logits(w.proj, s.bw, eg.src, eg.tgt, w.a, w.amax)
            ops.gat_agg_fwd(eg, w.proj, s.d, s.bf, w.a, w.amax, s.eps, out, w.wgt, w.den, act=act, ode=ode)
        elif self.raw_logits():
            ops.gat_logits_heads_raw(w.proj, eg.src, eg.tgt, s.heads, w.a, w.heads_scratch, bw=s.bw)
            ops.gat_agg_heads_fwd(eg, w.proj, s.o, w.bf0, w.a, w.heads_scratch, s.heads, s.eps, out.view(s.n * s.heads, s.o),
                                  w.wgt, w.den, act=act)
        else:
            ops.gat_logits_heads(w.proj, eg.src, eg.tgt, s.heads, w.a, bw=s.bw)
            ops.gat_agg_fwd(eg, w.proj, s.o, w.bf0, w.a, w.zero, s.eps, out.view(s.n * s.heads, s.o), w.wgt, w.den, act=act,
                            ode=ode)
        return terms

    def _kernel_act(self):
        """(act, ode) of the ops wrappers: (None, False) under relu messages."""
        if self.s.act[0] == ops.GAT_ACT_RELU:
            return None, False
        return self.s.act, True

    def eval(self, t, terms, out):
        self._forward(t, terms[0], out[0])


class GatOdeAdjointField(GatOdeField):
    """Components: [y, a, a_t, theta], theta laid out as GatOdeSpec.off."""

    def __init__(self, spec, work, order):
        super().__init__(spec, work)
        self.order = order
        self.n_components = 4
        self.ratio_groups = [[0], [1], [2], [3]]

    def new_state(self, y_end):
        s = self.s
        return [y_end.clone(), torch.zeros_like(y_end), torch.zeros(1, dtype=torch.float32, device=y_end.device),
                torch.zeros(s.n_theta, dtype=torch.float32, device=y_end.device)]

    def param_grads(self, comps):
        return theta_param_grads(self.s, self.order, comps[3])

    def dopri5_step_native(self, y, kk, y1, t, h, rtol, atol):
        lib = _lib.load()
        fs, ws = self._structs(True)
        arr = lambda c: (ctypes.c_void_p * 7)(*[kk[i][c].data_ptr() for i in range(7)])      # noqa: E731
        sums = torch.empty(4, dtype=torch.float64, device=y[0].device)
        _lib.check(lib.gode_gat_ode_dopri5_step_adjoint(
            ctypes.byref(fs), _lib.ptr(y[0]), _lib.ptr(y[1]), _lib.ptr(y[2]), _lib.ptr(y[3]), arr(0), arr(1), arr(2), arr(3),
            _lib.ptr(y1[0]), _lib.ptr(y1[1]), _lib.ptr(y1[2]), _lib.ptr(y1[3]), ctypes.byref(ws), float(t), float(h),
            float(rtol), float(atol), _lib.ptr(sums), _lib.ptr(self.w.err_scratch), _lib.stream_ptr()),
            "gode_gat_ode_dopri5_step_adjoint")
        return sums

    def _adjoint_parts(self, S):
        """S - 1 partial slots for a one-call adaptive step on the one-launch route (the sweeps' slots when they exist), else
        None: each stage then closes its own partials."""
        w = self.w
        if not self.small():
            return None
        if w.sweep is not None:
            return w.sweep.parts
        if w.adj_parts is None or w.adj_parts.numel() < (S - 1) * w.small_part.numel():
            w.adj_parts = torch.empty((S - 1) * w.small_part.numel(), dtype=torch.float32, device=w.small_part.device)
        return w.adj_parts

    def _adaptive_step_native(self, method, y, kk, y1, t, h, rtol, atol):
        """dopri5_step_native for any adaptive method: gode_gat_ode_adaptive_step_adjoint - on launch-bound graphs the S - 1
        stages' closing launches as one (gode_gat_small_finish_multi_f32), and one fused close for the four components."""
        lib = _lib.load()
        S = adaptive_stages(method)
        fs, ws = self._structs(True)
        arr = lambda c: (ctypes.c_void_p * S)(*[kk[i][c].data_ptr() for i in range(S)])      # noqa: E731
        sums = torch.empty(4, dtype=torch.float64, device=y[0].device)
        _lib.check(lib.gode_gat_ode_adaptive_step_adjoint(
            adaptive_code(method), ctypes.byref(fs), _lib.ptr(y[0]), _lib.ptr(y[1]), _lib.ptr(y[2]), _lib.ptr(y[3]), arr(0),
            arr(1), arr(2), arr(3), _lib.ptr(y1[0]), _lib.ptr(y1[1]), _lib.ptr(y1[2]), _lib.ptr(y1[3]), ctypes.byref(ws),
            _lib.ptr(self._adjoint_parts(S)), float(t), float(h), float(rtol), float(atol), _lib.ptr(sums),
            _lib.ptr(self.w.err_scratch), _lib.stream_ptr()), "gode_gat_ode_adaptive_step_adjoint")
        return sums

    # ---- fixed-grid steps on launch-bound graphs: the small components (a_t, theta) are advanced once per RK step ----
    deferred_components = (2, 3)
    DEFER_SMALL = True            # False: every stage closes its own partials (round 3)

    def begin_rk4_step(self):
        if not (self.DEFER_SMALL and self.small()):
            self._slots = None
            return False
        w = self.w
        if w.step_parts is None:
            w.step_parts = torch.empty(4 * w.small_part.numel(), dtype=torch.float32, device=w.small_part.device)
        self._slots = []              # evaluation times of the stages seen so far in this step
        return True

    def finish_rk4_step(self, weights, y):
        s, ts = self.s, self._slots
        self._slots = None
        ops.gat_small_finish_step(self.w.step_parts, s.n, s.d, s.heads, ts, weights[:len(ts)], y[3], y[2])
        return self.deferred_components

    def _stage_part(self, t):
        """Partial buffer of the stage being evaluated, and whether its closing launch is deferred to the end of the step."""
        slots = getattr(self, "_slots", None)
        if slots is None:
            return self.w.small_part, False
        k = len(slots)
        slots.append(t)
        n = self.w.small_part.numel()
        return self.w.step_parts[k * n:(k + 1) * n], True

    def eval(self, t, terms, out):
        s, w = self.s, self.w
        eg, n, d, o, H = s.eg, s.n, s.d, s.o, s.heads
        xt = self._forward(t, terms[0], out[0])
        g = s.views(out[3])
        raw = self.raw_logits()
        # cotangent -a of the VJP, masked by the outer relu, is formed inside the kernel
        act, ode = self._kernel_act()
        if H == 1:
            ops.gat_vjp(eg, w.proj, o, s.bf, w.a, w.amax, w.wgt, w.den, out[0], w.dz, w.da, w.dPs, w.dPt, w.dA2,
                        cot_terms=terms[1], cot_scale=-1.0, act=act, ode=ode)
        else:
            nv = n * H
            ops.gat_vjp(eg, w.proj, o, w.bf0, w.a, w.zero, w.wgt, w.den, out[0].view(nv, o), w.dz, w.da, w.dPs.view(nv, o),
                        w.dPt.view(nv, o), w.dA2.view(nv, 2), cot_terms=terms[1], cot_scale=-1.0, heads=H,
                        raw_scratch=w.heads_scratch if raw else None, defer_maxpath=raw, act=act, ode=ode)
        if self.small():
            # launch-bound graphs: k_a and the partials of every parameter gradient in one launch, one more to close (on the
            # raw-logit route the per-head max-path sums are taken off dA2 inside the first)
            part, deferred = self._stage_part(t)
            ops.gat_dense_vjp_small(xt, n, d, s.groups, s.eps_gn, s.gamma, s.beta, s.Wsrc, s.Wtgt, s.Wlog, H, w.dPs, w.dPt, w.dA2,
                                    out[1], part, maxfix=(w.heads_scratch, eg.src, eg.tgt) if raw and eg.E > 0 else None,
                                    packed=s.Wpacked)
            if not deferred:
                ops.gat_small_finish(part, n, d, H, t, out[3], out[2])
            return
        # bias gradients: sum over edges of dz / da = sum over nodes of the per-target sums just formed (every edge has
        # exactly one target) - N rows instead of E
        merged = n <= MERGED_FINISH_MAX_ROWS and s.groups > 0 and not s.pad_logits     # ONE reduction launch closes the stage
        if merged:
            n_a = ops.colsum_parts(w.dPt, w.colsum_scratch)
            n_b = ops.colsum_parts(w.dA2, w.colsum_scratch2)
        else:
            ops.colsum_(g["bf"], w.dPt)
            if H == 1:
                ops.colsum_(g["bw"], w.dA2[:, 1:2].contiguous())
            else:
                ops.colsum_(w.ba_grad, w.dA2)
                g["bw"].copy_(w.ba_grad[1::2])
        nb = w.np_b
        affine = s.groups > 0
        Wl, dAl = s.Wlog, w.dA2
        if s.pad_logits:
            w.dA2pad[:, :2 * H].copy_(w.dA2)
            Wl, dAl = s.Wlog_pad, w.dA2pad
        for j, (Wj, dPj) in enumerate(((s.Wsrc, w.dPs), (s.Wtgt, w.dPt), (Wl, dAl))):
            ops.gn_time_gemm_bwd(xt, n, d, s.groups, s.eps_gn, s.gamma, Wj, True, dPj, out=out[1],
                                 pre_terms=[(1.0, out[1])] if j else None,
                                 parts=(w.gp[j * nb:(j + 1) * nb], w.bp[j * nb:(j + 1) * nb]) if affine else None)
        if affine and not merged:
            ops.reduce_parts2_(g["gamma"], w.gp, g["beta"], w.bp)
        elif not affine:
            g["gamma"].zero_(); g["beta"].zero_()
        for j, dPj in enumerate((w.dPs, w.dPt, dAl)):
            ops.wgrad(xt, n, d, s.groups, s.eps_gn, s.gamma, s.beta, dPj, True, part=w.wp[j])
        if merged:
            i, npw = s.i, w.wp[0].shape[0]
            ops.reduce_segments_([
                (g["Wsrc"], w.wp[0], npw, i * d, 0, 1, i * d, s.Wsrc[0], d),          # row 0 of each block = its time row
                (g["Wtgt"], w.wp[1], npw, i * d, 0, 1, i * d, s.Wtgt[0], d),
                (g["Wlog"], w.wp[2], npw, i * 2 * H, 0, 1, i * 2 * H, s.Wlog[0], 2 * H),
                (g["bf"], w.colsum_scratch, n_a, d, 0, 1, d, None, 0),
                (g["bw"], w.colsum_scratch2, n_b, 2 * H, 1, 2, H, None, 0),           # the odd columns of the n x 2H sums
                (g["gamma"], w.gp, 3 * nb, d, 0, 1, d, None, 0),
                (g["beta"], w.bp, 3 * nb, d, 0, 1, d, None, 0)], t, out[2])
            return
        ops.reduce_parts2_(g["Wsrc"].view(-1), w.wp[0], g["Wtgt"].view(-1), w.wp[1])
        if s.pad_logits:
            ops.reduce_parts_(w.gWlog_pad.view(-1), w.wp[2])
            g["Wlog"].copy_(w.gWlog_pad[:, :2 * H])
        else:
            ops.reduce_parts_(g["Wlog"].view(-1), w.wp[2])
        # a_t' = -a^T df/dt over the three time rows; each row 0 *= t
        ops.time_row_fixup3_([g["Wsrc"][0], g["Wtgt"][0], g["Wlog"][0]], [s.Wsrc[0], s.Wtgt[0], s.Wlog[0]], t, out[2])


def gat_fields(odefunc, layer, eg, n, names, y0, act_layer=None):
    """Hook body of gat_models.ODEfunc.gode_fields and gat_heads.ODEfunc.gode_fields, after their own checks of the
    graph: the fused fields of relu(layer([t | odefunc.norm1(x)])) on n nodes, or None.  eg is the graph the kernels see
    (the H-fold graph with H heads); names maps id(parameter) -> its name in param_grads.  The message activation is
    act_layer.act (default: layer.act); one the kernels do not restate (a lambda, a custom module) has no fused field."""
    if message_activation((layer if act_layer is None else act_layer).act) is None or y0.dim() != 2 or n != y0.shape[0]:
        return None
    plist = [p for p in odefunc.parameters() if p.requires_grad]
    if len(plist) != len(names) or any(id(p) not in names for p in plist):
        return None
    spec = GatOdeSpec(eg, n, layer, odefunc.norm1, act_layer)
    # a one-head and an H-head function on the same edge list keep their own buffers
    key = ("heads", spec.d, y0.device) if spec.heads > 1 else (spec.d, y0.device)
    cache = eg.__dict__.setdefault("_ode_work", {})
    work = cache.get(key)
    if work is None:
        work = cache[key] = _Work(spec, y0.device)
    order = [names[id(p)] for p in plist]
    return GatOdeField(spec, work, order), (lambda: GatOdeAdjointField(spec, work, order)), tuple(plist)
