"""`odeint` / `odeint_adjoint` with the public torchdiffeq signature (the solver seam of
GCN/models.py:5,192, GAT/models.py:5,192 in the reference):

    odeint_adjoint(func, y0, t, rtol=1e-6, atol=1e-12, method=None, options=None)
        -> Tensor[len(t), *y0.shape]

`func` is an nn.Module called as func(t: 0-dim tensor, y).  When it offers
`gode_fields(y0)` (our ODEfunc does) the whole f-eval and its VJP run as fused HIP kernels
and stage inputs are never materialised; any other module runs through autograd with the
RK arithmetic still in the HIP kernels.

`odeint` is differentiable as torchdiffeq's is (backprop through the solver's operations, not the adjoint): with grad
mode on and y0 or a parameter of func requiring grad it returns a tensor with a grad_fn whose gradient is the exact
derivative of the computed discrete solution w.r.t. y0 and func's parameters (t gets None).  Under adaptive dopri5 the
accepted step sizes are constants of that derivative: rejected attempts, the initial-step heuristic and the controller
contribute nothing (what autograd through a solver whose step sizes are Python floats gives).  Row-partitioned fields
stay forward-only.
"""
import weakref

import torch

from . import ops
from . import solver
from .solver import (DP_A, DP_B, DP_C, DP_MID, Dopri5Record, Dopri5Stats, Field, integrate_dopri5,
                     integrate_dopri5_inplace, integrate_rk4, uniform_grid)


NATIVE_RK4 = True      # fused fields: issue a whole rk4 solve from one C-ABI call (False: per-stage Python driver)
# Fixed-grid solves of fused fields on launch-bound sizes (state of at most this many elements) are captured into a
# HIP graph the second time the same solve is requested and replayed afterwards; 0 turns the capture off.
GRAPH_CAPTURE_MAX_ELEMS = 1 << 21
# `nfe` after a backward pass is an integer the reference's harness prints (GCN/train_res.py:100-101).  torchdiffeq's
# adjoint evaluates func once more per output time for dL/dt before it integrates backwards; under fixed-grid rk4 that
# value can reach nothing the seam returns (the time gradient is discarded and a fixed grid never looks at it), so the
# evaluation is NOT executed here - but with this flag on (default) it is COUNTED, so that nfe_b reads 65 for 64 stage
# evaluations exactly as with torchdiffeq (asserted against the oracle's own count in tests/test_gpu_gcn.py).  Off:
# nfe counts the evaluations actually launched (64).  Adaptive dopri5 executes and counts the evaluation either way.
NFE_COUNTS_SKIPPED_DLDT_EVAL = True
# Backprop through a fused rk4 solve keeps y_n and k_1..k_4 of every step (5 n d floats per step) when they fit in this many
# bytes (2^20 x 128 state, 16 steps: 40 GiB); above it only y_n is kept and each step is re-run into a one-step record just
# before its reverse sweep (the same launches: gradients bit for bit those of the save-everything mode).
# Backprop through a fused dopri5 solve keeps y_n and k_1..k_7 of every accepted step (8 n d floats per step) under the same
# bound; a solve that outgrows it keeps y_n and k_1 and re-runs each step (one native step call) before its sweep.
BACKPROP_SAVE_MAX_BYTES = 48 << 30


def _materialise(terms):
    if len(terms) == 1 and terms[0][0] == 1.0:
        return terms[0][1]
    out = torch.empty_like(terms[0][1])
    return ops.lincomb_(out, terms)


class AutogradField(Field):
    """Forward field of an arbitrary module: one component."""
    n_components = 1

    def __init__(self, func, like):
        self.func = func
        self.like = like

    def eval(self, t, terms, out):
        y = _materialise(terms[0])
        tt = torch.tensor(t, dtype=self.like.dtype, device=self.like.device)
        with torch.no_grad():
            out[0].copy_(self.func(tt, y))


class AutogradAdjointField(Field):
    """Augmented field (y, a, a_t, theta...) of an arbitrary module via torch.autograd."""

    def __init__(self, func, params, like):
        self.func = func
        self.params = tuple(params)
        self.like = like
        self.n_components = 3 + len(self.params)
        self.ratio_groups = [[0], [1], [2]] + ([list(range(3, 3 + len(self.params)))] if self.params else [])

    def eval(self, t, terms, out):
        y = _materialise(terms[0])
        a = _materialise(terms[1])
        with torch.enable_grad():
            tt = torch.tensor(t, dtype=self.like.dtype, device=self.like.device, requires_grad=True)
            y_ = y.detach().requires_grad_(True)
            fe = self.func(tt, y_)
            vj = torch.autograd.grad(fe, (tt, y_) + self.params, -a, allow_unused=True)
        out[0].copy_(fe.detach())
        out[1].copy_(vj[1]) if vj[1] is not None else out[1].zero_()
        out[2].copy_(vj[0].reshape(out[2].shape)) if vj[0] is not None else out[2].zero_()
        for i, _p in enumerate(self.params):
            g = vj[2 + i]
            out[3 + i].copy_(g) if g is not None else out[3 + i].zero_()


def _check_state(y0):
    if not torch.is_tensor(y0):
        raise TypeError("graph_odenet_amd.odeint: y0 must be a tensor (tuple states are not part of the hot path)")
    if not y0.is_cuda:
        raise RuntimeError("graph_odenet_amd.odeint: y0 must live on the GPU (got %s); there is no CPU path" % y0.device)
    if y0.dtype != torch.float32:
        raise TypeError("graph_odenet_amd.odeint: y0 must be float32")


def _times(t):
    # The reference's ODEBlock keeps `integration_time` on the device (GCN/models.py:195 `type_as(x)`), so reading it
    # is a device->host copy = a host synchronisation in the middle of every forward pass (measured at C5: the GPU
    # then idles ~0.3 ms while the host catches up).  The values are remembered on the tensor object together with its
    # storage address and version counter, so only the first call (and any call after an in-place change or a
    # `set_` / `.data =` re-pointing) pays for it.  NOT seen: a write through an alias that bumps no version counter of
    # this tensor (`t.data.copy_(...)`, a raw kernel): pass the end points as Python floats or a CPU tensor then
    # (models.ODEBlock re-creates `integration_time` from its own floats on every forward, as the reference does).
    if torch.is_tensor(t) and t.is_cuda:
        hit = getattr(t, "_gode_times", None)
        key = (t.data_ptr(), t._version, tuple(t.shape))
        if hit is not None and hit[0] == key:
            tl = hit[1]
        else:
            tl = [float(v) for v in t.tolist()]
            try:
                t._gode_times = (key, tl)
            except Exception:
                pass
        tl = list(tl)
    else:
        tl = [float(v) for v in (t.tolist() if torch.is_tensor(t) else t)]
    if len(tl) < 2:
        raise ValueError("odeint: t must hold at least two time points")
    return tl


def _method(method):
    m = "dopri5" if method is None else method
    if m not in ("dopri5", "rk4"):
        raise ValueError("odeint: unsupported method %r (supported: dopri5, rk4)" % (method,))
    return m


def _integrate(field, comps, t0, t1, rtol, atol, method, options, stats):
    if method == "rk4":
        stats.nfe += _run_rk4(field, comps, t0, t1, uniform_grid(t0, t1, (options or {}).get("step_size")))
    else:
        if getattr(field, "fixed_grid_only", False):
            raise NotImplementedError("odeint: this field supports the fixed-grid method only (method='rk4')")
        if hasattr(field, "adaptive"):
            field.adaptive = True                  # row-partitioned fields: keep the small components global
        prep = getattr(field, "prepare", None)
        if prep is not None:
            prep()
        integrate_dopri5_inplace(field, comps, t0, t1, rtol, atol, stats)


class _GraphedSolve:
    """One captured fixed-grid solve: static input components, the HIP graph, and the components holding the result."""

    def __init__(self, field, comps, t0, t1, n_steps):
        from . import _lib
        lib = _lib.load()
        self.field = field
        self.inputs = list(comps)
        self.nfe = 4 * n_steps
        work = list(comps)
        overlap = lib.gode_get_option(b"overlap")
        lib.gode_set_option(b"overlap", 0)           # launch-bound sizes gain nothing from the second stream
        try:
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                _run_rk4(field, work, t0, t1, n_steps)
        finally:
            lib.gode_set_option(b"overlap", overlap)
        self.outputs = work

    def run(self, values):
        """values[c]: tensor copied into input component c, or None for zero.  Returns clones of the result."""
        for dst, src in zip(self.inputs, values):
            if src is None:
                dst.zero_()
            else:
                dst.copy_(src)
        self.graph.replay()
        return [o.clone() for o in self.outputs]


class _Plan:
    """Per-(func, problem) record: fields kept alive across training steps and their captured solves."""

    def __init__(self, fwd, mk_adj, plist):
        self.fwd, self.mk_adj, self.plist = fwd, mk_adj, plist
        self.adj = None
        self.seen_f = self.seen_b = 0
        self.gf = self.gb = None
        self.no_capture = False          # set when a capture attempt failed: the plan stays on the eager path


_PLANS = weakref.WeakKeyDictionary()      # func module -> {key: _Plan}; kept off the module so that deepcopy / pickling
                                          # of a model never meets a HIP graph


def plans_of(func):
    """The captured-solve plans of an ODE function module (created on first use)."""
    plans = _PLANS.get(func)
    if plans is None:
        plans = _PLANS[func] = {}
    return plans


def _try_capture(plan, field, comps, t0, t1):
    """A captured solve, or None (and the plan switched to the eager path for good) when the capture fails."""
    try:
        return _GraphedSolve(field, comps, t0, t1, plan.n_steps)
    except RuntimeError as exc:
        import warnings
        plan.no_capture = True
        warnings.warn("graph_odenet_amd: HIP-graph capture of a fixed-grid solve failed (%s); staying on the eager path"
                      % (str(exc).splitlines()[0],))
        return None


def _plan_for(func, y0, tl, method, options, params):
    """(plan, fields) of this solve; plan is None when the solve is not eligible for capture.  A func opts in by
    offering gode_plan_token(y0): a cheap hashable identity of everything the fields depend on besides the state
    shape and the parameter storage (i.e. the graph)."""
    tok = getattr(func, "gode_plan_token", None)
    token = None
    if (tok is not None and GRAPH_CAPTURE_MAX_ELEMS > 0 and method == "rk4" and len(tl) == 2
            and y0.numel() <= GRAPH_CAPTURE_MAX_ELEMS and not torch.cuda.is_current_stream_capturing()):
        token = tok(y0)
    if token is None:
        return None, _fields(func, y0)
    n = uniform_grid(tl[0], tl[1], (options or {}).get("step_size"))
    # the hook's identity is part of the key: a func whose gode_fields was swapped (e.g. to force the autograd path)
    # must not be served the fused fields of an earlier plan
    key = (tuple(y0.shape), y0.device.index, tl[0], tl[1], n, token, tuple(p.data_ptr() for p in params), NATIVE_RK4,
           id(getattr(func, "gode_fields", None).__func__) if hasattr(getattr(func, "gode_fields", None), "__func__") else None)
    plans = plans_of(func)
    plan = plans.get(key)
    if plan is None:
        fields = _fields(func, y0)
        if not getattr(fields[0], "fused", False):
            return None, fields
        if len(plans) >= 4:
            plans.clear()                       # a func that keeps changing graphs / shapes: start over
        plan = plans[key] = _Plan(*fields)
        plan.n_steps = n
    return plan, (plan.fwd, plan.mk_adj, plan.plist)


def _run_rk4(field, comps, t0, t1, n):
    prep = getattr(field, "prepare", None)
    if prep is not None:
        prep()
    native = getattr(field, "rk4_native", None)
    if native is not None and NATIVE_RK4:
        return native(comps, t0, t1, n)          # whole solve issued from C (csrc/ode_driver.hip)
    return integrate_rk4(field, comps, t0, t1, n)


def _extra_inputs(func):
    """Differentiable inputs of func that are not its parameters (private hook `gode_extra_inputs`, e.g. the edge
    matrices of qc_ode.EdgeODEfunc: the output of a trainable encoder).  Their gradients are returned after the
    parameters'; a func without the hook has none."""
    hook = getattr(func, "gode_extra_inputs", None)
    return tuple(hook()) if hook is not None else ()


def _params(func):
    """What a solve differentiates with respect to besides y0: func's trainable parameters, then its extra inputs."""
    params = tuple(p for p in func.parameters() if p.requires_grad) if isinstance(func, torch.nn.Module) else ()
    return params + _extra_inputs(func)


def _fields(func, y0):
    mk = getattr(func, "gode_fields", None)
    if mk is not None:
        pair = mk(y0)
        if pair is not None:
            return pair
    params = _params(func)
    return AutogradField(func, y0), (lambda: AutogradAdjointField(func, params, y0)), params


def _rows(field):
    """(order, inverse) when the field integrates on renumbered nodes (state rows y' = y[order]), else (None, None)."""
    return getattr(field, "row_order", None), getattr(field, "row_inverse", None)


def _bump_nfe(func, n):
    # fused fields do not call func.forward; keep the reference's counter (GCN/models.py:173) alive
    if getattr(func, "_gode_counts_nfe", False):
        func.nfe += n


def _rk4_torch(func, y, t0, t1, n):
    """n 3/8-rule steps from t0 to t1 as differentiable torch ops through func (torchdiffeq's rk4 step)."""
    h = (t1 - t0) / n
    tt = lambda v: torch.tensor(v, dtype=y.dtype, device=y.device)      # noqa: E731
    for i in range(n):
        t = t0 + i * h
        k1 = func(tt(t), y)
        k2 = func(tt(t + h / 3.0), y + h * k1 / 3.0)
        k3 = func(tt(t + 2.0 * h / 3.0), y + h * (k2 - k1 / 3.0))
        k4 = func(tt(t + h), y + h * (k1 - k2 + k3))
        y = y + (k1 + 3.0 * (k2 + k3) + k4) * (h * 0.125)
    return y


class _OdeintBackprop(torch.autograd.Function):
    """odeint under rk4 with gradients: the forward is odeint's own (bit for bit), the backward the exact derivative of
    the discrete solution.  Fused fields offering rk4_forward_save / rk4_backprop (GcnOdeField) keep the stage
    derivatives of every step and run the reverse sweep as one C call per interval (csrc/ode_driver.hip); any other field
    re-runs each interval as torch ops through func under autograd from its saved start state (what torchdiffeq does)."""

    @staticmethod
    def forward(ctx, func, fields, tl, rtol, atol, options, y0, *params):
        fwd = fields[0]
        order, inverse = _rows(fwd)
        step_size = (options or {}).get("step_size")
        steps = [uniform_grid(tl[i - 1], tl[i], step_size) for i in range(1, len(tl))]
        fused = getattr(fwd, "rk4_forward_save", None) is not None and NATIVE_RK4
        y0c = y0.detach().contiguous()
        outs = [y0c.clone()]
        ctx.saved = None
        with torch.no_grad():
            if fused:
                prep = getattr(fwd, "prepare", None)
                if prep is not None:
                    prep()
                shape = tuple(y0c.shape)
                save_all = 5 * sum(steps) * y0c.numel() * 4 <= BACKPROP_SAVE_MAX_BYTES
                cur = y0c.clone() if order is None else y0c.index_select(0, order)
                saved = []
                for i in range(1, len(tl)):
                    n = steps[i - 1]
                    y_end = torch.empty_like(cur)
                    if save_all:
                        rec = torch.empty((n, 5) + shape, dtype=y0c.dtype, device=y0c.device)
                        rec[0, 0].copy_(cur)
                        fwd.rk4_forward_save(rec[0, 0], y_end, rec, tl[i - 1], tl[i], n, 0, n)
                        saved.append(rec)
                    else:
                        ys = torch.empty((n,) + shape, dtype=y0c.dtype, device=y0c.device)
                        ys[0].copy_(cur)
                        rec = torch.empty((1, 5) + shape, dtype=y0c.dtype, device=y0c.device)
                        for j in range(n):
                            fwd.rk4_forward_save(ys[j], ys[j + 1] if j + 1 < n else y_end, rec, tl[i - 1], tl[i], n, j, j + 1)
                        saved.append(ys)
                    cur = y_end
                    outs.append(cur.clone() if order is None else cur.index_select(0, inverse))
                ctx.saved, ctx.save_all = saved, save_all
                _bump_nfe(func, 4 * sum(steps))
            else:
                stats = Dopri5Stats()
                ys = [y0c.clone() if order is None else y0c.index_select(0, order)]
                for i in range(1, len(tl)):
                    _integrate(fwd, ys, tl[i - 1], tl[i], rtol, atol, "rk4", options, stats)
                    outs.append(ys[0].clone() if order is None else ys[0].index_select(0, inverse))
                _bump_nfe(func, stats.nfe if getattr(fwd, "fused", False) else 0)
        ans = torch.stack(outs)
        ctx.func, ctx.fields, ctx.tl, ctx.steps, ctx.fused = func, fields, tl, steps, fused
        ctx.outs = None if fused else outs
        ctx.n_params = len(params)
        return ans

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous()
        tl, steps = ctx.tl, ctx.steps
        params = ctx.fields[2] if ctx.fused else _params(ctx.func)
        if ctx.fused:
            fwd = ctx.fields[0]
            order, inverse = _rows(fwd)
            gather = (lambda g: g.clone()) if order is None else (lambda g: g.index_select(0, order))
            a = gather(grad_out[-1])
            s = fwd.s
            d = s.d
            nW = (d + 1) * d
            theta = torch.zeros((nW + 3 * d + 1,), dtype=torch.float32, device=a.device)
            scratch = rec1 = None
            with torch.no_grad():
                for i in range(len(tl) - 1, 0, -1):
                    n, sv = steps[i - 1], ctx.saved[i - 1]
                    if ctx.save_all:
                        res = fwd.rk4_backprop(sv, a, theta, tl[i - 1], tl[i], n, 0, n)
                        if res is not a:
                            a.copy_(res)
                    else:
                        if rec1 is None:
                            rec1 = torch.empty((1, 5) + tuple(a.shape), dtype=a.dtype, device=a.device)
                            scratch = torch.empty_like(a)
                        for j in range(n - 1, -1, -1):          # re-run the step into a one-step record, then sweep it
                            fwd.rk4_forward_save(sv[j], scratch, rec1, tl[i - 1], tl[i], n, j, j + 1)
                            res = fwd.rk4_backprop(rec1, a, theta, tl[i - 1], tl[i], n, j, j + 1)
                            if res is not a:
                                a.copy_(res)
                    if i > 1:
                        a.add_(gather(grad_out[i - 1]))
                gy0 = (a if order is None else a.index_select(0, inverse)).add_(grad_out[0])
            comps = [None, None, None, theta[:nW].view(d + 1, d), theta[nW:nW + d], theta[nW + d:nW + 2 * d],
                     theta[nW + 2 * d:nW + 3 * d]]
            pg = ctx.fields[1]().param_grads(comps)
        else:
            func = ctx.func
            nfe0 = getattr(func, "nfe", None)
            a = grad_out[-1]
            pg = [None] * len(params)
            for i in range(len(tl) - 1, 0, -1):
                with torch.enable_grad():
                    y = ctx.outs[i - 1].detach().requires_grad_(True)
                    yt = _rk4_torch(func, y, tl[i - 1], tl[i], steps[i - 1])
                    g = torch.autograd.grad(yt, (y,) + tuple(params), a, allow_unused=True)
                a = g[0] + grad_out[i - 1] if g[0] is not None else grad_out[i - 1].clone()
                for q, gq in enumerate(g[1:]):
                    if gq is not None:
                        pg[q] = gq if pg[q] is None else pg[q] + gq
            gy0 = a
            if nfe0 is not None:
                func.nfe = nfe0                   # evaluations re-run by the backward pass are not counted (torchdiffeq's
                                                  # odeint counts none in its backward)
        return (None, None, None, None, None, None, gy0, *pg)


def _interp_weights(x):
    """(cy0, cy1, kc[7]): the 4th-order interpolation at abscissa x of a step as cy0 y_n + cy1 y_{n+1} + h sum kc_s k_s
    (solver.integrate_dopri5 forms the same numbers)."""
    x2, x3, x4 = x * x, x * x * x, x * x * x * x
    wm = 16 * x4 - 32 * x3 + 16 * x2
    cy0 = -8 * x4 + 18 * x3 - 11 * x2 + 1 + wm
    cy1 = -8 * x4 + 14 * x3 - 5 * x2
    kc = [wm * m for m in DP_MID]
    kc[0] += -2 * x4 + 5 * x3 - 4 * x2 + x
    kc[6] += 2 * x4 - 3 * x3 + x2
    return cy0, cy1, kc


def _dopri5_step_torch(func, y, t, h, x):
    """One Dormand-Prince step from y at t as differentiable torch ops through func; x: the interpolation abscissa of a
    last step that overshot the end time (None: the step's own end state is returned)."""
    tt = lambda v: torch.tensor(v, dtype=y.dtype, device=y.device)      # noqa: E731
    ks = [func(tt(t), y)]
    for s in range(1, 7 if x is not None else 6):       # k_7 enters the result through the interpolation only
        ks.append(func(tt(t + DP_C[s] * h), y + sum((h * a) * k for a, k in zip(DP_A[s], ks) if a != 0.0)))
    y1 = y + sum((h * b) * k for b, k in zip(DP_B, ks) if b != 0.0)
    if x is None:
        return y1
    cy0, cy1, kc = _interp_weights(x)
    return cy0 * y + cy1 * y1 + sum((h * c) * k for c, k in zip(kc, ks) if c != 0.0)


class _OdeintBackpropDopri5(torch.autograd.Function):
    """odeint under adaptive dopri5 with gradients: the forward is odeint's own (bit for bit, the same launches on buffers
    a solver.Dopri5Record keeps), the backward the exact derivative of the discrete solution with the accepted step
    sizes as constants.  A fused field offering dopri5_step_backprop (GcnOdeField) keeps y_n and k_1..k_7 of every
    accepted step - or y_n and k_1 past BACKPROP_SAVE_MAX_BYTES, each step then re-run by one native step call before
    its sweep - and sweeps them in reverse, one C call per step (csrc/ode_driver.hip).  Any other field keeps y_n and
    re-runs each accepted step as torch ops through func under autograd, k_1 = func(t_n, y_n) recomputed: the same
    function of y_n as the derivative FSAL hands over, since Y_7 and y_{n+1} are the same combination."""

    @staticmethod
    def forward(ctx, func, fields, tl, rtol, atol, y0, *params):
        fwd = fields[0]
        order, inverse = _rows(fwd)
        fused = getattr(fwd, "dopri5_step_backprop", None) is not None and solver.DOPRI5_NATIVE
        if getattr(fwd, "fixed_grid_only", False):
            raise NotImplementedError("odeint: this field supports the fixed-grid method only (method='rk4')")
        y0c = y0.detach().contiguous()
        outs = [y0c.clone()]
        stats = Dopri5Stats()
        records = []
        with torch.no_grad():
            prep = getattr(fwd, "prepare", None)
            if prep is not None:
                prep()
            cur = y0c.clone() if order is None else y0c.index_select(0, order)
            left = BACKPROP_SAVE_MAX_BYTES
            for i in range(1, len(tl)):
                rec = Dopri5Record(7, left) if fused and left is not None else Dopri5Record(1 if fused else 0)
                (cur,), _ = integrate_dopri5(fwd, [cur], tl[i - 1], tl[i], rtol, atol, stats, record=rec)
                if fused and left is not None:
                    left = left - rec.bytes if rec.keep == 7 else None      # past the bound: the later intervals keep k_1 only
                records.append(rec)
                outs.append(cur.clone() if order is None else cur.index_select(0, inverse))
        _bump_nfe(func, stats.nfe if getattr(fwd, "fused", False) else 0)
        ctx.func, ctx.fields, ctx.tl, ctx.tols, ctx.fused, ctx.records = func, fields, tl, (rtol, atol), fused, records
        return torch.stack(outs)

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous()
        tl, records = ctx.tl, ctx.records
        fwd = ctx.fields[0]
        order, inverse = _rows(fwd)
        if ctx.fused:
            gather = (lambda g: g.clone()) if order is None else (lambda g: g.index_select(0, order))
            a = gather(grad_out[-1])
            d = fwd.s.d
            nW = (d + 1) * d
            theta = torch.zeros((nW + 3 * d + 1,), dtype=torch.float32, device=a.device)
            work = fwd.dopri5_backprop_work(a)
            rerun = None
            turn = 0                                    # which (ybar_n, kbar_1) pair the next call writes: never the one it reads
            with torch.no_grad():
                for i in range(len(tl) - 1, 0, -1):
                    steps = records[i - 1].steps
                    kbar7 = None
                    for j in range(len(steps) - 1, -1, -1):
                        t, h, x, y, ks = steps[j]
                        ks = [k[0] for k in ks]
                        if len(ks) < 7:                 # re-run the step into a one-step record (the forward's launches)
                            if rerun is None:
                                rerun = [torch.empty_like(a) for _ in range(7)]
                            fwd.dopri5_step_native(y, [[ks[0]]] + [[b] for b in rerun[:6]], [rerun[6]], t, h, *ctx.tols)
                            ks = [ks[0]] + rerun[:6]
                        if x is None:
                            wy, wk = 1.0, [h * b for b in DP_B]
                        else:
                            cy0, cy1, kc = _interp_weights(x)
                            wy, wk = cy0 + cy1, [h * (cy1 * b + c) for b, c in zip(DP_B, kc)]
                        a, kbar7 = fwd.dopri5_step_backprop(y[0], ks, a, kbar7, wy, wk, t, h, j == 0, work, turn, theta)
                        turn ^= 1
                    if i > 1:
                        a = a.add_(gather(grad_out[i - 1]))
                gy0 = (a.clone() if order is None else a.index_select(0, inverse)).add_(grad_out[0])
            comps = [None, None, None, theta[:nW].view(d + 1, d), theta[nW:nW + d], theta[nW + d:nW + 2 * d],
                     theta[nW + 2 * d:nW + 3 * d]]
            pg = ctx.fields[1]().param_grads(comps)
        else:
            func = ctx.func
            params = _params(func)
            nfe0 = getattr(func, "nfe", None)
            a = grad_out[-1]
            pg = [None] * len(params)
            for i in range(len(tl) - 1, 0, -1):
                for (t, h, x, y, _) in reversed(records[i - 1].steps):
                    with torch.enable_grad():
                        yn = (y[0] if order is None else y[0].index_select(0, inverse)).detach().requires_grad_(True)
                        g = torch.autograd.grad(_dopri5_step_torch(func, yn, t, h, x), (yn,) + tuple(params), a,
                                                allow_unused=True)
                    a = g[0] if g[0] is not None else torch.zeros_like(a)
                    for q, gq in enumerate(g[1:]):
                        if gq is not None:
                            pg[q] = gq if pg[q] is None else pg[q] + gq
                a = a + grad_out[i - 1]
            gy0 = a
            if nfe0 is not None:
                func.nfe = nfe0                   # evaluations re-run by the backward pass are not counted
        return (None, None, None, None, None, gy0, *pg)


def odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None):
    """torchdiffeq's odeint.  With grad mode on and y0 or a parameter of func requiring grad the result is differentiable
    (backprop through the solve: _OdeintBackprop under rk4, _OdeintBackpropDopri5 under dopri5; t gets no gradient);
    otherwise - and always on row-partitioned fields - a forward solve without gradient support."""
    _check_state(y0)
    tl = _times(t)
    method = _method(method)
    fields = _fields(func, y0)
    fwd = fields[0]
    if torch.is_grad_enabled() and getattr(fwd, "big_components", None) is None:
        params = _params(func)
        if y0.requires_grad or params:
            same = len(fields[2]) == len(params) and all(p is q for p, q in zip(fields[2], params))
            hook = "rk4_forward_save" if method == "rk4" else "dopri5_step_backprop"
            if getattr(fwd, hook, None) is not None and not same:
                fields = (AutogradField(func, y0), None, params)      # the fused field does not cover these parameters
            if method != "rk4":
                return _OdeintBackpropDopri5.apply(func, fields, tl, float(rtol), float(atol), y0, *params)
            return _OdeintBackprop.apply(func, fields, tl, float(rtol), float(atol), options, y0, *params)
    stats = Dopri5Stats()
    order, inverse = _rows(fwd)
    ys = [y0.detach().contiguous().clone() if order is None else y0.detach().index_select(0, order)]
    outs = [y0.detach().contiguous().clone()]
    with torch.no_grad():
        for i in range(1, len(tl)):
            _integrate(fwd, ys, tl[i - 1], tl[i], rtol, atol, method, options, stats)
            outs.append(ys[0].clone() if order is None else ys[0].index_select(0, inverse))
    _bump_nfe(func, stats.nfe if getattr(fwd, "fused", False) else 0)
    return torch.stack(outs)


class _OdeintAdjoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, func, tl, rtol, atol, method, options, last_only, y0, *params):
        plan, (fwd, mk_adj, plist) = _plan_for(func, y0, tl, method, options, params)
        stats = Dopri5Stats()
        order, inverse = _rows(fwd)
        y0c = y0.detach().contiguous()
        # ans_p[i] = state at tl[i] in the field's row order (what the adjoint starts from); every slice is written in
        # place - the start by the renumbering gather, each later one by the integrator working on that slice - so a
        # solve moves the state through memory twice around the integration instead of once per clone and stack
        # (at 2^20 x 128 a pass is 0.2 ms; the clone-and-stack form made ten of them per forward pass)
        ans_p = torch.empty((len(tl),) + tuple(y0c.shape), dtype=y0c.dtype, device=y0c.device)
        if order is None:
            ans_p[0].copy_(y0c)
        else:
            torch.index_select(y0c, 0, order, out=ans_p[0])     # state rows in the renumbered graph's order
        if plan is not None and plan.gf is None and plan.seen_f >= 1 and not plan.no_capture:
            plan.gf = _try_capture(plan, fwd, [ans_p[0].clone()], tl[0], tl[1])
        if plan is not None and plan.gf is not None:
            (y_end,) = plan.gf.run([ans_p[0]])
            stats.nfe += plan.gf.nfe
            ans_p[1].copy_(y_end)
        else:
            for i in range(1, len(tl)):
                ans_p[i].copy_(ans_p[i - 1])
                ys = [ans_p[i]]
                _integrate(fwd, ys, tl[i - 1], tl[i], rtol, atol, method, options, stats)
                if ys[0].data_ptr() != ans_p[i].data_ptr():       # an integrator that returns a new tensor
                    ans_p[i].copy_(ys[0])
            if plan is not None:
                plan.seen_f += 1
        _bump_nfe(func, stats.nfe if getattr(fwd, "fused", False) else 0)
        ctx.last_only = bool(last_only)
        if last_only:
            # only y(t[-1]) leaves (what the reference's ODEBlock keeps, GCN/models.py:200 `out[1]`): no copy of y0 into
            # a stacked result, and the backward pass gets the cotangent of that one state instead of a zero-filled stack
            ans = ans_p[-1].clone() if order is None else torch.index_select(ans_p[-1], 0, inverse)
        elif order is None:
            ans = ans_p
        else:
            ans = torch.empty_like(ans_p)
            ans[0].copy_(y0c)
            for i in range(1, len(tl)):
                torch.index_select(ans_p[i], 0, inverse, out=ans[i])
        ctx.func, ctx.tl, ctx.rtol, ctx.atol, ctx.method, ctx.options = func, tl, rtol, atol, method, options
        ctx.mk_adj = mk_adj
        ctx.fwd = fwd
        ctx.plan = plan
        ctx.n_params = len(params)
        ctx.rows = (order, inverse)
        ctx.save_for_backward(ans_p)
        return ans

    @staticmethod
    def backward(ctx, grad_out):
        (ans,) = ctx.saved_tensors
        func, tl = ctx.func, ctx.tl
        grad_out = grad_out.contiguous()
        order, inverse = ctx.rows
        back = (lambda g: g) if order is None else (lambda g: g.index_select(0, inverse))
        last_only = ctx.last_only
        n_t = len(tl)

        def g_raw(i):                                 # dL/dy(tl[i]) in the caller's row order, None = zero
            if last_only:
                return grad_out if i in (n_t - 1, -1) else None
            return grad_out[i]

        def g_at(i):                                  # the same in the field's row order (one gather, when asked for)
            g = g_raw(i)
            return g if (g is None or order is None) else g.index_select(0, order)

        def add_start(g):                             # + cotangent of the start state, rows already in the caller's order
            g0 = g_raw(0) if n_t > 1 else None
            return g if g0 is None else g.add_(g0)
        plan = ctx.plan
        if plan is not None and plan.seen_b >= 1 and plan.gb is None and not plan.no_capture:
            with torch.no_grad():
                plan.adj = plan.mk_adj()
                plan.gb = _try_capture(plan, plan.adj, plan.adj.new_state(ans[1]), tl[1], tl[0])
        if plan is not None and plan.gb is not None:
            with torch.no_grad():
                vals = [ans[1], g_at(1)] + [None] * (len(plan.gb.inputs) - 2)
                comps = plan.gb.run(vals)
                gy0 = add_start(back(comps[1]))
            _bump_nfe(func, plan.gb.nfe + ((n_t - 1) if NFE_COUNTS_SKIPPED_DLDT_EVAL else 0))
            return (None, None, None, None, None, None, None, gy0, *plan.adj.param_grads(comps))
        if plan is not None:
            plan.seen_b += 1
        adj = ctx.mk_adj()
        fwd = ctx.fwd
        ctx_tmp = torch.empty_like(ans[0])
        stats = Dopri5Stats()
        with torch.no_grad():
            comps = adj.new_state(ans[-1]) if hasattr(adj, "new_state") else None
            if comps is None:
                comps = [ans[-1].clone(), torch.zeros_like(ans[-1]),
                         torch.zeros(1, dtype=ans.dtype, device=ans.device)]
                comps += [torch.zeros_like(p) for p in adj.params]
            if order is None:
                comps[1].copy_(g_raw(-1))
            else:
                torch.index_select(g_raw(-1), 0, order, out=comps[1])
            for i in range(len(tl) - 1, 0, -1):
                comps[0].copy_(ans[i])
                if ctx.method != "rk4":
                    # dL/dt at the output time enters the adaptive error control (torchdiffeq evaluates
                    # func once more here); a fixed grid never looks at it, so rk4 skips the eval.
                    fwd.eval(tl[i], [[(1.0, ans[i])]], [ctx_tmp])
                    stats.nfe += 1
                    gi = g_at(i)
                    if gi is not None:
                        comps[2].sub_((ctx_tmp * gi).sum().reshape(1))
                    if getattr(adj, "adaptive", None) is not None:
                        adj.adaptive = True
                        adj.reduce_small(comps[2])      # row-partitioned: a_t is a sum over all rows
                _integrate(adj, comps, tl[i], tl[i - 1], ctx.rtol, ctx.atol, ctx.method, ctx.options, stats)
                if i > 1 and g_raw(i - 1) is not None:
                    comps[1].add_(g_at(i - 1))
            # the cotangent of the start state is added after the rows are back in the caller's order: one pass, and
            # no gather of a slice that is all zeros whenever the loss only looks at the end state
            gy0 = add_start(back(comps[1]))
        skipped = (n_t - 1) if (ctx.method == "rk4" and NFE_COUNTS_SKIPPED_DLDT_EVAL) else 0
        _bump_nfe(func, (stats.nfe if getattr(adj, "fused", False) else 0) + skipped)
        pg = adj.param_grads(comps) if hasattr(adj, "param_grads") else comps[3:]
        return (None, None, None, None, None, None, None, gy0, *pg)


def odeint_adjoint(func, y0, t, rtol=1e-6, atol=1e-12, method=None, options=None, _last_only=False):
    """torchdiffeq's odeint_adjoint for the two solvers of the hot path.  `_last_only=True` (not part of the reference
    API; used by models.ODEBlock, which keeps `out[1]` only) returns y(t[-1]) instead of the stack over t."""
    _check_state(y0)
    tl = _times(t)
    method = _method(method)
    if not isinstance(func, torch.nn.Module):
        raise ValueError("odeint_adjoint: func must be an nn.Module")
    params = _params(func)
    return _OdeintAdjoint.apply(func, tl, float(rtol), float(atol), method, options, bool(_last_only), y0, *params)
