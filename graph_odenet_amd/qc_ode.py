"""Continuous-depth edge-conditioned block of the QM9 models: the reference's ODEfunc / ODEBlock pair
(GCN/models.py:161-201) with the QC layer (QC/layers.py:114-154) in place of the GCN layer,

    f(t, x) = relu(EdgeGraphConvolution([t | GroupNorm(x)], Esrc, Etgt, edge_data)),

and its fused fields.  Per evaluation at the stage input X = sum of (coef, tensor) terms:

    S = [t | GN(X)] W                              gode_gn_time_gemm_f32                          (1 launch)
    f = relu(Etgt . bmm(A, S[Esrc]) + b)           gode_edge_ode_feval_f32                        (1 launch; from
        ops.EDGE_ODE_FUSED_MAX_EDGES edges on: gode_edge_matvec_msg_f32 + SpMM with the bias / relu epilogue, 2 launches)

and for the adjoint field, cotangent g = -a masked by f > 0:

    dM = g,  dS = Ms_inc . (A_e^T (val_e dM[tgt_e]))     gode_edge_ode_vjp_f32                    (1 launch; large: + SpMM)
    a' = GroupNorm / time / GEMM VJP of dS               gode_gn_time_gemm_bwd_f32                (1 launch)
    dW partials                                          gode_wgrad_f32                           (1 launch)
    theta' = [dW | db = colsum(dM) | dgamma | dbeta], a_t'   gode_reduce_segments_f32             (1 launch)
    A' : dA_e = (val_e dM[tgt_e]) (x) S[src_e]           gode_edge_outer_sum_acc_f32

The adjoint integrates [y, a, a_t, theta, a_A]: theta = [W | b | gamma | beta] packed in one buffer, a_A of E h^2 floats.
`edge_data` is an INPUT of the ODE function (the output of the trainable edge encoder), not one of its parameters; it
reaches the autograd Functions of odeint.py through the private hook `gode_extra_inputs` and its gradient is returned
after the parameters'.

Error-ratio groups (dopri5): y, a, a_t, and theta TOGETHER WITH a_A.  torchdiffeq integrates the adjoint of everything
it returns a gradient for as ONE flat tensor (its f_params); the only way it returns dL/d(edge_data) at all is with
edge_data among func's parameters - which is also how the tests' oracle gets it - so a_A is counted with the parameters.

Backprop through the solve (odeint, adjoint=False) on launch-bound batches: the forward records k_s of every stage (the last
rk4 stage through gode_edge_ode_feval_save_f32), so the reverse of a stage evaluates nothing again:

    dM, dS, Ybar_s, the rows' dgamma / dbeta shares, S      gode_edge_ode_stage_bwd_f32            (1 launch)
    dW partials                                              gode_wgrad_f32                         (1 launch)

and a step of S swept stages ends with ONE gode_edge_ode_step_close_f32 (parameter gradients of all its stages into the
packed buffer [W | b | gamma | beta | a_A]), ONE gode_edge_outer_sum_acc_f32 over its (dM_s, S_s) pairs when edge_data asks
for a gradient, and at most one combine of the cotangent: 2 S + 3 launches.  Larger batches keep the generic path (the
interval re-run as torch ops under autograd).

Under fixed-grid rk4 the four stages of a step share A: each stage keeps its (dM, S) pair (N x h each) and ONE
gode_edge_outer_sum_acc_f32 pass per step applies the RK weights and adds into a_A (solver.integrate_rk4's
begin_rk4_step / finish_rk4_step); a_A then has no stage buffers and no RK combine.  Under dopri5 every stage writes
its own dA into its stage buffer.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .functional import GroupNorm
from .qc_layers import EdgeGraphConvolution, _edges, _EdgeSet
from .solver import ADAPTIVE_TABLEAUS, FIXED_METHODS, FIXED_TABLEAUS, MULTISTEP_METHODS, Field, _stage_terms


def _edge_index(Esrc, Etgt):
    """(target index [E] int64, value [E]) of Etgt in any of its forms, as plain torch (the CPU / non-fp32 path)."""
    E = Esrc.numel()
    if isinstance(Etgt, _EdgeSet):
        row, val = Etgt.edge_row.to(torch.int64), Etgt.edge_val
        return row.clamp(min=0), torch.where(row >= 0, val, torch.zeros_like(val))
    if Etgt.layout == torch.strided:
        nz = Etgt != 0
        tgt = nz.to(torch.uint8).argmax(0)
        return tgt, Etgt.gather(0, tgt.unsqueeze(0)).squeeze(0)
    co = Etgt.coalesce()
    rows, cols = co.indices()
    tgt = torch.zeros(E, dtype=torch.int64, device=Esrc.device)
    val = torch.zeros(E, dtype=co.values().dtype, device=Esrc.device)
    tgt[cols] = rows
    val[cols] = co.values()
    return tgt, val


class EdgeODEfunc(nn.Module):
    """f(t, x) = relu(gc1([t | norm1(x)], Esrc, Etgt, edge_data)), counting calls in `nfe` (GCN/models.py:161-179 on the
    QC layer)."""

    _gode_counts_nfe = True
    FUSED = True                 # False: gode_fields declines (generic autograd fields)
    fixed_grid = False           # set by EdgeODEBlock: under rk4 the deferred a_A needs no stage buffers

    def __init__(self, dim):
        super().__init__()
        self.norm1 = GroupNorm(min(32, dim), dim)
        self.gc1 = EdgeGraphConvolution(dim + 1, dim)
        self.nfe = 0
        self.Esrc = self.Etgt = self.edge_data = None

    def set_edges(self, Esrc, Etgt, edge_data):
        self.Esrc, self.Etgt, self.edge_data = Esrc, Etgt, edge_data

    def forward(self, t, x):
        self.nfe += 1
        tt = torch.ones(x.shape[0], 1, dtype=x.dtype, device=x.device) * t
        if x.is_cuda and x.dtype == torch.float32:
            xx = torch.cat([tt, self.norm1(x)], 1)
            return F.relu(self.gc1(xx, self.Esrc, self.Etgt, self.edge_data))
        # plain torch (CPU, float64): the same formulas without the library
        n1, gc = self.norm1, self.gc1
        xx = torch.cat([tt, F.group_norm(x, n1.num_groups, n1.weight, n1.bias, n1.eps)], 1)
        S = torch.mm(xx, gc.weight)
        msg = torch.bmm(self.edge_data, S.index_select(0, self.Esrc).unsqueeze(-1)).squeeze(-1)
        tgt, val = _edge_index(self.Esrc, self.Etgt)
        M = torch.zeros(x.shape[0], gc.out_features, dtype=x.dtype, device=x.device).index_add_(0, tgt, val.unsqueeze(1) * msg)
        return F.relu(M + gc.bias if gc.bias is not None else M)

    def gode_extra_inputs(self):
        """Differentiable inputs of f besides its parameters (odeint.py appends their gradients after the parameters')."""
        A = self.edge_data
        return (A,) if (A is not None and A.requires_grad) else ()

    def gode_fields(self, y0):
        """Hook for graph_odenet_amd.odeint: (forward field, adjoint-field factory, plist) or None -> autograd fields."""
        A = self.edge_data
        if not self.FUSED or self.gc1.bias is None or y0.dim() != 2 or A is None or not y0.is_cuda:
            return None
        plist = [p for p in self.parameters() if p.requires_grad]
        if len(plist) != 4:
            return None                                  # frozen parameters
        d = self.gc1.out_features
        if y0.shape[1] != d or A.dim() != 3 or tuple(A.shape[1:]) != (d, d) or A.dtype != torch.float32 or \
                not ops.edge_ode_supported(d):
            return None
        es = _edges(self.Esrc, self.Etgt)
        if es.n != y0.shape[0] or es.E != A.shape[0] or es.E == 0:
            return None
        spec = EdgeOdeSpec(es, A.detach().contiguous(), self.gc1, self.norm1)
        work = _Work(spec, y0.device)
        names = {id(self.norm1.weight): "gamma", id(self.norm1.bias): "beta", id(self.gc1.weight): "W", id(self.gc1.bias): "b"}
        order = [names[id(p)] for p in plist]
        want_A, fixed = A.requires_grad, self.fixed_grid
        return EdgeOdeField(spec, work, order, want_A), (lambda: EdgeOdeAdjointField(spec, work, order, want_A, fixed)), tuple(plist)


class EdgeOdeSpec:
    """relu(layer([t | norm(x)])) on one batch: es (qc_layers._EdgeSet), A (E x d x d), theta = [W | b | gamma | beta]."""

    def __init__(self, es, A, layer, norm):
        self.es, self.A, self.n, self.d = es, A, es.n, layer.out_features
        self.W, self.b = layer.weight.detach(), layer.bias.detach()
        self.gamma, self.beta = norm.weight.detach(), norm.bias.detach()
        self.groups, self.eps = int(norm.num_groups), float(norm.eps)
        d = self.d
        self.off, p = {}, 0
        for name, ln in (("W", (d + 1) * d), ("b", d), ("gamma", d), ("beta", d)):
            self.off[name] = (p, p + ln)
            p += ln
        self.n_theta = p
        self.large = es.E >= ops.EDGE_ODE_FUSED_MAX_EDGES

    def views(self, theta):
        v = {k: theta[a:b] for k, (a, b) in self.off.items()}
        v["W"] = v["W"].view(self.d + 1, self.d)
        return v


class _Work:
    """Buffers of one batch (the batch changes with every training step, so they live as long as the fields)."""

    def __init__(self, spec, device):
        n, d, E = spec.n, spec.d, spec.es.E
        lib = _lib.load()
        f = dict(dtype=torch.float32, device=device)
        self.X = torch.empty(n, d, **f)
        self.S4, self.dM4 = torch.empty(4, n, d, **f), torch.empty(4, n, d, **f)      # one (dM, S) pair per stage of a step
        self.dS = torch.empty(n, d, **f)
        self.msg = torch.empty(E, d, **f) if spec.large else None                      # messages forward, dxe backward
        self.np_b, self.np_w = lib.gode_gemm_bwd_parts(n), lib.gode_wgrad_parts(n)
        self.gp, self.bp = torch.empty(self.np_b, d, **f), torch.empty(self.np_b, d, **f)
        self.wp = torch.empty(self.np_w, (d + 1) * d, **f)
        self.colsum_scratch = torch.empty(max(lib.gode_colsum_scratch_bytes(n, d), 16), dtype=torch.uint8, device=device)


class _BackpropWork:
    """Buffers of a reverse sweep: per swept stage of a step (dopri5: up to 7) the (dM, S) pair, the rows' dgamma / dbeta
    shares and the wgrad partials, which the step's closing launches read; one dS; the four Ybar of an rk4 step."""
    STAGES = 7

    def __init__(self, spec, device, want_S):
        n, d, q = spec.n, spec.d, self.STAGES
        f = dict(dtype=torch.float32, device=device)
        self.dM, self.gr, self.br = torch.empty(q, n, d, **f), torch.empty(q, n, d, **f), torch.empty(q, n, d, **f)
        self.S = torch.empty(q, n, d, **f) if want_S else None
        self.wp = torch.empty(q, _lib.load().gode_wgrad_parts(n), (d + 1) * d, **f)
        self.dS = torch.empty(n, d, **f)
        self.ybar = [torch.empty(n, d, **f) for _ in range(4)]


class EdgeOdeField(Field):
    """The forward field.  eval_combine folds the solution combine y + h sum b_s k_s of a fixed-grid step into the launch
    that ends its last stage.  Built with the parameter order (gode_fields) on a launch-bound batch it also offers the
    backprop half of the protocol (solver.Field); it has no dopri5_step_native / adaptive_step_native, so an adaptive record keeps all S k_s
    (seven under dopri5).
    Memory of that half: packed_param_grads hands out views of the one packed buffer, so as long as a parameter's .grad is
    such a view the whole buffer stays alive, its E h^2 edge-matrix tail included; and the field is rebuilt with every
    batch, so every odeint call that is backpropagated allocates a _BackpropWork (7 x 3 or 4 n x d arrays and 7 sets of
    wgrad partials).  Both are small at the launch-bound sizes this half is limited to (under 4 096 edges)."""
    n_components = 1
    fused = True
    BIAS_DIRECT_MAX_ROWS = 1024      # up to here the rows of dM are the bias gradient's partials; above, block partials first
    BACKPROP_FUSED = True            # False: no backprop members (odeint re-runs each interval as torch ops under autograd)

    def __init__(self, spec, work, order=None, want_A=False):
        self.s, self.w = spec, work
        self.slot = 0
        if order is not None and self.BACKPROP_FUSED and not spec.large and \
                ops.edge_ode_stage_bwd_supported(spec.n, spec.d, spec.groups):
            self.order, self.want_A, self._bwork = order, bool(want_A), None
            self.rk4_forward_save, self.rk4_backprop = self._rk4_forward_save, self._rk4_backprop
            self.fixed_forward_save, self.fixed_backprop = self._fixed_forward_save, self._fixed_backprop
            self.dopri5_step_backprop, self.dopri5_backprop_work = self._dopri5_step_backprop, self._dopri5_backprop_work
            self.adaptive_step_backprop, self.adaptive_backprop_work = self._adaptive_step_backprop, self._adaptive_backprop_work
            self.packed_grads, self.packed_param_grads = self._packed_grads, self._packed_param_grads

    # ---- backprop through the solve (odeint._OdeintBackprop): launch-bound batches -----------------------------------------
    def _packed_grads(self, device):
        """Zeroed [W | b | gamma | beta | a_A (E h^2, only when edge_data asks for a gradient)]."""
        s = self.s
        return torch.zeros(s.n_theta + (s.A.numel() if self.want_A else 0), dtype=torch.float32, device=device)

    def _packed_param_grads(self, theta):
        """The gradients in func.parameters() order, then edge_data's (E x h x h)."""
        s = self.s
        v = s.views(theta)
        return [v[k] for k in self.order] + ([theta[s.n_theta:].view_as(s.A)] if self.want_A else [])

    def _bw(self, device):
        if self._bwork is None:
            self._bwork = _BackpropWork(self.s, device, self.want_A)
        return self._bwork

    def _stage_bwd(self, q, cot, k, yin, t, ybar):
        """The reverse of one stage k = f(t, sum yin) with cotangent terms cot, into slot q of the step's buffers: 2 launches.
        Returns what the step's closing launch needs of it."""
        s, es, b = self.s, self.s.es, self._bw(k.device)
        ops.edge_ode_stage_bwd(es.Ms_inc, es.edge_row, es.edge_val, s.A, cot, 1.0, k, yin, t, s.gamma, s.beta, s.W, s.groups,
                               s.eps, b.dM[q], b.dS, ybar, b.gr[q], b.br[q], S=b.S[q] if self.want_A else None)
        ops.wgrad(yin, s.n, s.d, s.groups, s.eps, s.gamma, s.beta, b.dS, True, part=b.wp[q])
        return (b.wp[q], b.dM[q], b.gr[q], b.br[q], t)

    def _close_step(self, stages, theta):
        """theta += the parameter gradients of the step's swept stages (1 launch) and the edge-matrix gradient (1 launch)."""
        s, es, b = self.s, self.s.es, self._bwork
        ops.edge_ode_step_close(stages, s.n, s.d, theta)
        if self.want_A:
            ops.edge_outer_sum_acc(es.edge_row, es.edge_val, es.src, [(b.dM[q], b.S[q]) for q in range(len(stages))],
                                   [1.0] * len(stages), theta[s.n_theta:].view_as(s.A), True)

    def _rk4_forward_save(self, y0, y_end, save, t0, t1, n_steps, i0, i1):
        self._fixed_forward_save("rk4", y0, y_end, save, t0, t1, n_steps, i0, i1)

    def _rk4_backprop(self, save, a, theta, t0, t1, n_steps, i0, i1):
        return self._fixed_backprop("rk4", save, a, theta, t0, t1, n_steps, i0, i1)

    def _fixed_forward_save(self, method, y0, y_end, save, t0, t1, n_steps, i0, i1):
        """Steps i0 .. i1-1 with the launches of solver.integrate_fixed on this field (the same bits; rk4: integrate_rk4's);
        save[r] = [y_n, k_1..k_S] of step i0 + r, k_S stored by the launch that folds the last stage into the solution."""
        C, A, B = FIXED_TABLEAUS[method]
        L = len(C) - 1
        if y0.data_ptr() != save[0, 0].data_ptr():
            save[0, 0].copy_(y0)
        h = (t1 - t0) / n_steps
        for i in range(i0, i1):
            rec = save[i - i0]
            y, ks = [rec[0]], [[rec[1 + q]] for q in range(L + 1)]
            t = t0 + i * h
            for q in range(L):
                self.eval(t + C[q] * h, _stage_terms(y, ks, A[q], h), ks[q])
            pre = [(1.0, y[0])] + [(h * B[q], ks[q][0]) for q in range(L) if B[q] != 0.0]
            y_next = save[i - i0 + 1, 0] if i + 1 < i1 else y_end
            self._forward(t + C[L] * h, _stage_terms(y, ks, A[L], h)[0], y_next, pre=pre, alpha=h * B[L], k_out=ks[L][0])

    def _fixed_backprop(self, method, save, a, theta, t0, t1, n_steps, i0, i1):
        """Reverse sweep over the records of steps i0 .. i1-1: kbar_s = h b_s a + h sum_{r > s} a_rs Ybar_r (zero coefficients
        dropped), Ybar_s through the stage, a += sum_s Ybar_s.  `a` is advanced in place and returned."""
        C, A, B = FIXED_TABLEAUS[method]
        S = len(C)
        h = (t1 - t0) / n_steps
        yb = self._bw(a.device).ybar[:S]
        for i in range(i1 - 1, i0 - 1, -1):
            rec = save[i - i0]
            y, ks = [rec[0]], [[rec[1 + q]] for q in range(S)]
            t = t0 + i * h
            stages = []
            for q in range(S - 1, -1, -1):
                cot = ([(h * B[q], a)] if B[q] != 0.0 else []) + \
                      [(h * A[r][q], yb[r]) for r in range(q + 1, S) if A[r][q] != 0.0]
                stages.append(self._stage_bwd(len(stages), cot, ks[q][0], _stage_terms(y, ks, A[q], h)[0],
                                              t + C[q] * h, yb[q]))
            self._close_step(stages, theta)
            ops.lincomb_(a, [(1.0, a)] + [(1.0, b) for b in yb])
        return a

    def _dopri5_backprop_work(self, like):
        """Work arrays of dopri5_step_backprop: 7 Ybar and two (ybar_n, kbar_1) pairs that take turns from step to step."""
        return self._adaptive_backprop_work("dopri5", like)

    def _dopri5_step_backprop(self, y, k, g, kbar7, wy, wk, t, h, first, work, turn, theta):
        """_adaptive_step_backprop under the dopri5 tableau: the launches this member has always issued, in their order."""
        return self._adaptive_step_backprop("dopri5", y, k, g, kbar7, wy, wk, t, h, first, work, turn, theta)

    def _adaptive_backprop_work(self, method, like):
        """Work arrays of adaptive_step_backprop: S Ybar and two (ybar_n, kbar_1) pairs that take turns from step to step."""
        S = len(ADAPTIVE_TABLEAUS[method][0])
        return {"ybar": [torch.empty_like(like) for _ in range(S)],
                "pairs": [(torch.empty_like(like), torch.empty_like(like)) for _ in range(2)]}

    def _adaptive_step_backprop(self, method, y, k, g, kbar_last, wy, wk, t, h, first, work, turn, theta):
        """Reverse sweep over one accepted step of an adaptive method (S stages, tableau c, a), the algebra of
        gode_gcn_ode_adaptive_step_backprop (csrc/ode_driver.hip): kbar_s = wk[s] g + h sum_{r > s} a_rs Ybar_r (+ kbar_last on
        the last stage), Ybar_s through the stage for s = S..2 (and 1 when `first`), ybar_n = wy g + sum Ybar_s; a stage whose
        cotangent has no term is skipped.  Returns (ybar_n, kbar_1) in work["pairs"][turn]; kbar_1 is None when `first`."""
        C, A = ADAPTIVE_TABLEAUS[method][:2]
        S = len(C)
        ybar = work["ybar"]
        ybar_n, kbar1 = work["pairs"][turn]
        swept = [False] * S

        def cotangent(q):
            c = [(wk[q], g)] if wk[q] != 0.0 else []
            c += [(h * A[r][q], ybar[r]) for r in range(q + 1, S) if A[r][q] != 0.0 and swept[r]]
            return c + [(1.0, kbar_last)] if (q == S - 1 and kbar_last is not None) else c
        stages = []
        for q in range(S - 1, -1 if first else 0, -1):
            cot = cotangent(q)
            if not cot:
                continue
            yin = _stage_terms([y], [[x] for x in k], A[q], h)[0]
            stages.append(self._stage_bwd(len(stages), cot, k[q], yin, t + C[q] * h, ybar[q]))
            swept[q] = True
        pre = [(wy, g)] + [(1.0, ybar[q]) for q in range(S) if swept[q]]
        c0 = None if first else cotangent(0)
        if c0:
            ops.lincomb_multi_([ybar_n, kbar1], [pre, c0])
        else:
            ops.lincomb_(ybar_n, pre)
            if not first:
                kbar1.zero_()
        if stages:
            self._close_step(stages, theta)
        return ybar_n, (None if first else kbar1)

    def _forward(self, t, y_terms, out, pre=None, alpha=1.0, k_out=None):
        s, w, es = self.s, self.w, self.s.es
        S = w.S4[self.slot]
        x_out = w.X if (len(y_terms) > 1 and self.n_components > 1) else None
        ops.gn_time_gemm(y_terms, s.n, s.d, s.groups, s.eps, s.gamma, s.beta, s.W, True, t, out=S, x_out=x_out)
        if s.large:
            lib = _lib.load()
            _lib.check(lib.gode_edge_matvec_msg_f32(_lib.ptr(es.src), _lib.ptr(s.A), _lib.ptr(S), s.d, s.d, es.E, _lib.ptr(w.msg),
                                                    _lib.stream_ptr()), "gode_edge_matvec_msg_f32")
            ops.spmm(es.Mt, w.msg, bias=s.b, relu=True, out=out, pre_terms=pre, alpha=alpha)
        else:
            ops.edge_ode_feval(es.Mt, es.src, s.A, S, s.b, out, pre_terms=pre, alpha=alpha, k_out=k_out)
        return [(1.0, w.X)] if x_out is not None else y_terms

    def eval(self, t, terms, out):
        self._forward(t, terms[0], out[0])

    def eval_combine(self, t, terms, pre, alpha, out):
        self._forward(t, terms[0], out[0], pre=pre[0], alpha=alpha)
        return (0,)


class EdgeOdeAdjointField(EdgeOdeField):
    """Components [y, a, a_t, theta, a_A] (a_A only when edge_data asks for a gradient)."""
    eval_combine = None              # the adjoint stages need k_y itself (the relu mask), not the combined solution
    DEFER_EDGE_GRAD = True           # False: every rk4 stage writes its own dA and a_A is combined like any component
    deferred_components = (4,)

    def __init__(self, spec, work, order, want_A=True, fixed_grid=False):
        super().__init__(spec, work)
        self.order, self.want_A, self.fixed_grid = order, bool(want_A), bool(fixed_grid)
        self.n_components = 5 if self.want_A else 4
        self.ratio_groups = [[0], [1], [2], [3, 4] if self.want_A else [3]]
        self._deferred = False

    def new_state(self, y_end):
        s = self.s
        f = dict(dtype=torch.float32, device=y_end.device)
        st = [y_end.clone(), torch.zeros_like(y_end), torch.zeros(1, **f), torch.zeros(s.n_theta, **f)]
        return st + [torch.zeros_like(s.A)] if self.want_A else st

    def alloc_like(self, y, n):
        """Work copies of the state; under fixed-grid rk4 with the deferred edge-matrix gradient no stage reads or writes
        its a_A slot, so the n copies share one placeholder instead of n arrays of E h^2 floats."""
        share = self.want_A and self.fixed_grid and self.DEFER_EDGE_GRAD
        hold = torch.empty(1, dtype=torch.float32, device=y[0].device) if share else None
        return [[hold if (share and c == 4) else torch.empty_like(t) for c, t in enumerate(y)] for _ in range(n)]

    def param_grads(self, comps):
        v = self.s.views(comps[3])
        m = {k: v[k].clone() for k in ("W", "b", "gamma", "beta")}
        return [m[k] for k in self.order] + ([comps[4]] if self.want_A else [])

    # ---- fixed-grid steps: the four (dM, S) pairs of a step are closed by one outer-sum pass ---------------------------
    def begin_rk4_step(self):
        self._deferred = self.want_A and self.DEFER_EDGE_GRAD
        self.slot = 0
        return self._deferred

    def finish_rk4_step(self, weights, y):
        s, w, es, k = self.s, self.w, self.s.es, self.slot
        self._deferred, self.slot = False, 0
        ops.edge_outer_sum_acc(es.edge_row, es.edge_val, es.src, [(w.dM4[q], w.S4[q]) for q in range(k)], weights[:k], y[4], True)
        return self.deferred_components

    def eval(self, t, terms, out):
        s, w, es = self.s, self.w, self.s.es
        n, d = s.n, s.d
        xt = self._forward(t, terms[0], out[0])
        S, dM = w.S4[self.slot], w.dM4[self.slot]
        # cotangent -a of the VJP, masked by the relu, is formed inside the kernel
        if s.large:
            ops.edge_ode_vjp(None, es.edge_row, es.edge_val, s.A, terms[1], -1.0, out[0], dM, dxe=w.msg)
            ops.spmm(es.Ms_inc, w.msg, out=w.dS)
        else:
            ops.edge_ode_vjp(es.Ms_inc, es.edge_row, es.edge_val, s.A, terms[1], -1.0, out[0], dM, dS=w.dS)
        affine = s.groups > 0
        ops.gn_time_gemm_bwd(xt, n, d, s.groups, s.eps, s.gamma, s.W, True, w.dS, out=out[1],
                             parts=(w.gp, w.bp) if affine else None)
        ops.wgrad(xt, n, d, s.groups, s.eps, s.gamma, s.beta, w.dS, True, part=w.wp)
        g = s.views(out[3])
        i = d + 1
        if n <= self.BIAS_DIRECT_MAX_ROWS:
            bias_seg = (g["b"], dM, n, d, 0, 1, d, None, 0)
        else:
            bias_seg = (g["b"], w.colsum_scratch, ops.colsum_parts(dM, w.colsum_scratch), d, 0, 1, d, None, 0)
        segs = [(g["W"], w.wp, w.np_w, i * d, 0, 1, i * d, s.W[0], d), bias_seg]       # row 0 of W = its time row
        if affine:
            segs += [(g["gamma"], w.gp, w.np_b, d, 0, 1, d, None, 0), (g["beta"], w.bp, w.np_b, d, 0, 1, d, None, 0)]
        else:
            g["gamma"].zero_(); g["beta"].zero_()
        ops.reduce_segments_(segs, t, out[2])
        if self.want_A:
            if self._deferred:
                self.slot += 1
            else:
                ops.edge_outer_sum_acc(es.edge_row, es.edge_val, es.src, [(dM, S)], [1.0], out[4], False)


class EdgeODEBlock(nn.Module):
    """y(1) of y' = odefunc(t, y), y(0) = x on the edges (Esrc, Etgt, edge_data) (GCN/models.py:181-201 on the QC layer).
    `Etgt`: the dense N x E matrix, a sparse one, or qc_layers.prepared_edges(...).  The gradient reaches x, the
    parameters of `odefunc` and edge_data."""

    def __init__(self, odefunc, tol=1e-5, method=None, step_size=None, adjoint=True):
        super().__init__()
        self.odefunc = odefunc
        self.adjoint = bool(adjoint)       # False: odeint, differentiable by backprop through the solve (every method)
        self.integration_time = torch.tensor([0, 1]).float()
        self.tol, self.method, self.step_size = tol, method, step_size

    def forward(self, x, Esrc, Etgt, edge_data):
        from .odeint import odeint, odeint_adjoint
        self.integration_time = self.integration_time.type_as(x)
        self.odefunc.set_edges(Esrc, Etgt, edge_data)
        self.odefunc.fixed_grid = self.method in FIXED_METHODS or self.method in MULTISTEP_METHODS
        options = None if self.step_size is None else {"step_size": self.step_size}
        if not self.adjoint:
            return odeint(self.odefunc, x, self.integration_time, rtol=self.tol, atol=self.tol, method=self.method,
                          options=options)[1]
        return odeint_adjoint(self.odefunc, x, self.integration_time, rtol=self.tol, atol=self.tol, method=self.method,
                              options=options, _last_only=True)

    @property
    def nfe(self):
        return self.odefunc.nfe

    @nfe.setter
    def nfe(self, value):
        self.odefunc.nfe = value
