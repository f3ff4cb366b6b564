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
from .solver import Field


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
        return EdgeOdeField(spec, work), (lambda: EdgeOdeAdjointField(spec, work, order, want_A, fixed)), tuple(plist)


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


class EdgeOdeField(Field):
    """The forward field.  eval_combine folds the solution combine y + h sum b_s k_s of a fixed-grid step into the launch
    that ends its last stage."""
    n_components = 1
    fused = True
    BIAS_DIRECT_MAX_ROWS = 1024      # up to here the rows of dM are the bias gradient's partials; above, block partials first

    def __init__(self, spec, work):
        self.s, self.w = spec, work
        self.slot = 0

    def _forward(self, t, y_terms, out, pre=None, alpha=1.0):
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
            ops.edge_ode_feval(es.Mt, es.src, s.A, S, s.b, out, pre_terms=pre, alpha=alpha)
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
        self.adjoint = bool(adjoint)       # False: odeint, differentiable by backprop through the solve (rk4 and dopri5)
        self.integration_time = torch.tensor([0, 1]).float()
        self.tol, self.method, self.step_size = tol, method, step_size

    def forward(self, x, Esrc, Etgt, edge_data):
        from .odeint import odeint, odeint_adjoint
        self.integration_time = self.integration_time.type_as(x)
        self.odefunc.set_edges(Esrc, Etgt, edge_data)
        self.odefunc.fixed_grid = self.method == "rk4"
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
