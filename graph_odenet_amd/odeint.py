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
derivative of the computed discrete solution w.r.t. y0 and func's parameters (t gets None).  Methods: adaptive `dopri5`
(the default), `bosh3` and `adaptive_heun`, and the fixed-grid `rk4` (3/8 rule), `midpoint` and `euler` on the grid options['step_size'] gives (one step
per interval of t without it); euler at step_size 1/K is the weight-tied K-layer residual stack.  `explicit_adams` (4th-order
Adams-Bashforth) runs on the same grid: three rk4 start-up steps per interval of t, then one evaluation per step; a grid of at
most three steps per interval is the rk4 solve.  Under the adaptive methods the
accepted step sizes are constants of that derivative: rejected attempts, the initial-step heuristic and the controller
contribute nothing (what autograd through a solver whose step sizes are Python floats gives).  Row-partitioned fields
stay forward-only.
"""
import weakref

import torch

from . import ops
from . import solver
from .solver import (ADAPTIVE_METHODS, ADAPTIVE_TABLEAUS, FIXED_METHODS, FIXED_TABLEAUS, MULTISTEP_BETAS, MULTISTEP_METHODS,
                     Dopri5Record, Dopri5Stats, Field, adaptive_interp_weights, adaptive_stages, integrate_adaptive,
                     integrate_dopri5_inplace, integrate_fixed, integrate_multistep, integrate_rk4, multistep_nfe, n_stages,
                     uniform_grid)


NATIVE_RK4 = True      # fused fields: issue a whole fixed-grid solve from one C-ABI call (False: per-stage Python driver)
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
# bound; a solve that outgrows it keeps y_n and k_1 and re-runs each step (one native step call) before its sweep.  A field
# with a sweep but no dopri5_step_native (qc_ode.EdgeOdeField) has nothing to re-run a step with and keeps all seven always.
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

    def new_state(self, y_end):
        return [y_end.clone(), torch.zeros_like(y_end), torch.zeros(1, dtype=y_end.dtype, device=y_end.device)] + \
               [torch.zeros_like(p) for p in self.params]

    def param_grads(self, comps):
        return comps[3:]

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


# adaptive dopri5; fixed-grid rk4 (3/8 rule), euler, midpoint; adaptive bosh3 (Bogacki-Shampine 3(2)), adaptive_heun (2(1))
METHODS = ("dopri5",) + FIXED_METHODS + tuple(m for m in ADAPTIVE_METHODS if m != "dopri5")


# ... and the multistep ones (explicit_adams: 4th-order Adams-Bashforth, rk4 start-up).  GRID_METHODS: every method that runs
# on the uniform grid of options['step_size'] and never looks at dL/dt or the tolerances
GRID_METHODS = FIXED_METHODS + MULTISTEP_METHODS


def _method(method):
    m = "dopri5" if method is None else method
    if m not in METHODS and m not in MULTISTEP_METHODS:
        raise ValueError("odeint: unsupported method %r (supported: %s)" % (method, ", ".join(METHODS + MULTISTEP_METHODS)))
    return m


def _grid_method(method, tl, options):
    """A multistep method on intervals of at most K - 1 steps each never leaves its rk4 start-up: the solve IS the rk4 solve
    of that grid, and runs as one (every native path, sweep and captured plan of rk4; bit for bit its results)."""
    if method in MULTISTEP_METHODS:
        step_size = (options or {}).get("step_size")
        if all(uniform_grid(tl[i - 1], tl[i], step_size) < len(MULTISTEP_BETAS[method]) for i in range(1, len(tl))):
            return "rk4"
    return method


def _grid_nfe(method, n):
    """Evaluations of an n-step solve of one interval under a method of GRID_METHODS."""
    return multistep_nfe(method, n) if method in MULTISTEP_METHODS else n_stages(method) * n


def _integrate(field, comps, t0, t1, rtol, atol, method, options, stats):
    if method == "rk4":
        stats.nfe += _run_rk4(field, comps, t0, t1, uniform_grid(t0, t1, (options or {}).get("step_size")))
    elif method in GRID_METHODS:
        stats.nfe += _run_fixed(field, comps, t0, t1, uniform_grid(t0, t1, (options or {}).get("step_size")), method)
    else:
        if field.fixed_grid_only:
            raise NotImplementedError(_FIXED_ONLY)
        if field.big_components is not None:
            field.adaptive = True                  # row-partitioned fields: keep the small components global
        _prepare(field)
        integrate_dopri5_inplace(field, comps, t0, t1, rtol, atol, stats, method)


_FIXED_ONLY = "odeint: this field supports the fixed-grid methods only (method=%s)" % " / ".join(
    repr(m) for m in GRID_METHODS)


class _GraphedSolve:
    """One captured fixed-grid solve: static input components, the HIP graph, and the components holding the result."""

    def __init__(self, field, comps, t0, t1, n_steps, method="rk4"):
        from . import _lib
        lib = _lib.load()
        self.field = field
        self.inputs = list(comps)
        self.nfe = _grid_nfe(method, n_steps)
        work = list(comps)
        overlap = lib.gode_get_option(b"overlap")
        lib.gode_set_option(b"overlap", 0)           # launch-bound sizes gain nothing from the second stream
        try:
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                _run_fixed(field, work, t0, t1, n_steps, method)
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
        return _GraphedSolve(field, comps, t0, t1, plan.n_steps, plan.method)
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
    if (tok is not None and GRAPH_CAPTURE_MAX_ELEMS > 0 and method in GRID_METHODS and len(tl) == 2
            and y0.numel() <= GRAPH_CAPTURE_MAX_ELEMS and not torch.cuda.is_current_stream_capturing()):
        token = tok(y0)
    if token is None:
        return None, _fields(func, y0)
    n = uniform_grid(tl[0], tl[1], (options or {}).get("step_size"))
    # the hook's identity is part of the key: a func whose gode_fields was swapped (e.g. to force the autograd path)
    # must not be served the fused fields of an earlier plan
    # ... and the method: an euler solve after an rk4 solve of the same func must not replay the rk4 graph
    key = (tuple(y0.shape), y0.device.index, tl[0], tl[1], n, method, token, tuple(p.data_ptr() for p in params), NATIVE_RK4,
           id(getattr(func, "gode_fields", None).__func__) if hasattr(getattr(func, "gode_fields", None), "__func__") else None)
    plans = plans_of(func)
    plan = plans.get(key)
    if plan is None:
        fields = _fields(func, y0)
        if not fields[0].fused:
            return None, fields
        if len(plans) >= 4:
            plans.clear()                       # a func that keeps changing graphs / shapes: start over
        plan = plans[key] = _Plan(*fields)
        plan.n_steps, plan.method = n, method
    return plan, (plan.fwd, plan.mk_adj, plan.plist)


def _run_rk4(field, comps, t0, t1, n):
    _prepare(field)
    if field.rk4_native is not None and NATIVE_RK4:
        return field.rk4_native(comps, t0, t1, n)          # whole solve issued from C (csrc/ode_driver.hip)
    return integrate_rk4(field, comps, t0, t1, n)


def _run_multistep(field, comps, t0, t1, n, method):
    """A solve of one interval by a method of solver.MULTISTEP_BETAS; at most K - 1 steps: _run_rk4's launches exactly."""
    if n < len(MULTISTEP_BETAS[method]):
        return _run_rk4(field, comps, t0, t1, n)
    _prepare(field)
    if field.multistep_native is not None and NATIVE_RK4:
        nfe = field.multistep_native(comps, t0, t1, n, method)     # whole solve issued from C; None: not on that route
        if nfe is not None:
            return nfe
    return integrate_multistep(field, comps, t0, t1, n, method)


def _run_fixed(field, comps, t0, t1, n, method):
    """A uniform-grid solve by any method of GRID_METHODS; rk4 takes _run_rk4's launches exactly."""
    if method == "rk4":
        return _run_rk4(field, comps, t0, t1, n)
    if method in MULTISTEP_METHODS:
        return _run_multistep(field, comps, t0, t1, n, method)
    _prepare(field)
    if field.fixed_native is not None and NATIVE_RK4:
        nfe = field.fixed_native(comps, t0, t1, n, method)     # whole solve issued from C; None: not on that route
        if nfe is not None:
            return nfe
    return integrate_fixed(field, comps, t0, t1, n, method)


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


def _prepare(field):
    if field.prepare is not None:
        field.prepare()


def _gather(y, index, out=None, copy=True):
    """y[index]: the state rows into (index = field.row_order) or out of (field.row_inverse) a field's order; index is
    None on a field that integrates the rows as given - then y itself with copy=False, else a copy.  out: written in
    place."""
    if index is not None:
        return torch.index_select(y, 0, index, out=out)
    if out is not None:
        return out.copy_(y)
    return y.clone() if copy else y


def _bump_nfe(func, field, n, skipped=0):
    # fused fields do not call func.forward; keep the reference's counter (GCN/models.py:173) alive.  skipped: evaluations
    # counted whichever field ran (NFE_COUNTS_SKIPPED_DLDT_EVAL)
    if getattr(func, "_gode_counts_nfe", False):
        func.nfe += (n if field.fused else 0) + skipped


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


def _fixed_torch(func, y, t0, t1, n, method):
    """n steps of a fixed-grid method from t0 to t1 as differentiable torch ops through func; rk4 is _rk4_torch."""
    if method == "rk4":
        return _rk4_torch(func, y, t0, t1, n)
    C, A, B = FIXED_TABLEAUS[method]
    h = (t1 - t0) / n
    tt = lambda v: torch.tensor(v, dtype=y.dtype, device=y.device)      # noqa: E731
    for i in range(n):
        t = t0 + i * h
        ks = []
        for s in range(len(C)):
            ks.append(func(tt(t + C[s] * h), y + sum((h * a) * k for a, k in zip(A[s], ks) if a != 0.0)))
        y = y + sum((h * b) * k for b, k in zip(B, ks) if b != 0.0)
    return y


def _multistep_torch(func, y, t0, t1, n, method):
    """n steps of a multistep method from t0 to t1 as differentiable torch ops through func: _rk4_torch's step for the
    start-up, k_1 kept; then one evaluation per step.  Autograd through it gives f_i the cotangent of every later step that
    reads it, on top of what k_1 gets inside its own rk4 step."""
    beta = MULTISTEP_BETAS[method]
    K = len(beta)
    if n < K:
        return _rk4_torch(func, y, t0, t1, n)
    h = (t1 - t0) / n
    tt = lambda v: torch.tensor(v, dtype=y.dtype, device=y.device)      # noqa: E731
    fs = []                                                              # f_{i-1}, f_{i-2}, ... (newest first)
    for i in range(n):
        t = t0 + i * h
        k1 = func(tt(t), y)
        fs.insert(0, k1)
        if i < K - 1:
            k2 = func(tt(t + h / 3.0), y + h * k1 / 3.0)
            k3 = func(tt(t + 2.0 * h / 3.0), y + h * (k2 - k1 / 3.0))
            k4 = func(tt(t + h), y + h * (k1 - k2 + k3))
            y = y + (k1 + 3.0 * (k2 + k3) + k4) * (h * 0.125)
        else:
            y = y + sum((h * b) * f for b, f in zip(beta, fs))
            fs.pop()
    return y


def _dopri5_step_torch(func, y, t, h, x, method="dopri5"):
    """One step of an adaptive method (FSAL form) from y at t as differentiable torch ops through func; x: the interpolation
    abscissa of a last step that overshot the end time (None: the step's own end state is returned)."""
    C, A, B = ADAPTIVE_TABLEAUS[method][:3]
    S = len(C)
    tt = lambda v: torch.tensor(v, dtype=y.dtype, device=y.device)      # noqa: E731
    ks = [func(tt(t), y)]
    for s in range(1, S if x is not None else S - 1):   # k_S enters the result through the interpolation only
        ks.append(func(tt(t + C[s] * h), y + sum((h * a) * k for a, k in zip(A[s], ks) if a != 0.0)))
    y1 = y + sum((h * b) * k for b, k in zip(B, ks) if b != 0.0)
    if x is None:
        return y1
    cy0, cy1, kc = adaptive_interp_weights(method, x)
    return cy0 * y + cy1 * y1 + sum((h * c) * k for c, k in zip(kc, ks) if c != 0.0)


def _fixed_sweep(fwd, method):
    """(forward_save, backprop) of a field under a fixed-grid method, both taking (.., t0, t1, n, i0, i1) - or None.  rk4
    keeps the members it has always used."""
    if method == "rk4":
        if fwd.rk4_forward_save is None:
            return None
        return fwd.rk4_forward_save, fwd.rk4_backprop
    if fwd.fixed_forward_save is None:
        return None
    return (lambda *args: fwd.fixed_forward_save(method, *args)), (lambda *args: fwd.fixed_backprop(method, *args))


class _Rk4Backprop:
    """What _OdeintBackprop does per interval under a fixed-grid method of S stages (rk4, euler, midpoint).  Fused (a field
    offering rk4_forward_save / rk4_backprop, for the other methods fixed_forward_save / fixed_backprop: GcnOdeField): the
    record is [y_n, k_1..k_S] of every step, swept in reverse by one C call per interval (csrc/ode_driver.hip) - or, when
    the whole solve outgrows BACKPROP_SAVE_MAX_BYTES, y_n alone, each step then re-run into a one-step record just before
    its sweep.  Generic: the record is the interval's start state, from which the interval is re-run as torch ops through
    func (what torchdiffeq does)."""
    own_cotangent = True              # fused_reverse hands back the tensor it was given

    def __init__(self, func, fwd, tl, rtol, atol, options, y0c, method="rk4"):
        self.func, self.fwd, self.tl, self.tols, self.options = func, fwd, tl, (rtol, atol), options
        self.method, self.S = method, n_stages(method)
        step_size = (options or {}).get("step_size")
        self.steps = [uniform_grid(tl[i - 1], tl[i], step_size) for i in range(1, len(tl))]
        sweep = _fixed_sweep(fwd, method) if NATIVE_RK4 else None
        self.fused = sweep is not None
        self.stats = Dopri5Stats()
        if self.fused:
            self.forward_save, self.backprop = sweep
            _prepare(fwd)
            self.save_all = (self.S + 1) * sum(self.steps) * y0c.numel() * 4 <= BACKPROP_SAVE_MAX_BYTES

    def forward(self, i, cur, start):
        fwd, t0, t1, n = self.fwd, self.tl[i - 1], self.tl[i], self.steps[i - 1]
        if not self.fused:
            ys = [cur]
            _integrate(fwd, ys, t0, t1, *self.tols, self.method, self.options, self.stats)
            return start, ys[0]
        shape, like = tuple(cur.shape), dict(dtype=cur.dtype, device=cur.device)
        y_end = torch.empty_like(cur)
        if self.save_all:
            rec = torch.empty((n, self.S + 1) + shape, **like)
            rec[0, 0].copy_(cur)
            self.forward_save(rec[0, 0], y_end, rec, t0, t1, n, 0, n)
        else:
            rec = torch.empty((n,) + shape, **like)
            rec[0].copy_(cur)
            one = torch.empty((1, self.S + 1) + shape, **like)
            for j in range(n):
                self.forward_save(rec[j], rec[j + 1] if j + 1 < n else y_end, one, t0, t1, n, j, j + 1)
        self.stats.nfe += self.S * n
        return rec, y_end

    def fused_reverse(self, i, rec, a, theta, work):
        t0, t1, n = self.tl[i - 1], self.tl[i], self.steps[i - 1]
        if self.save_all:
            res = self.backprop(rec, a, theta, t0, t1, n, 0, n)
            if res is not a:
                a.copy_(res)
            return a
        if not work:
            work.update(one=torch.empty((1, self.S + 1) + tuple(a.shape), dtype=a.dtype, device=a.device),
                        y=torch.empty_like(a))
        for j in range(n - 1, -1, -1):          # re-run the step into a one-step record, then sweep it
            self.forward_save(rec[j], work["y"], work["one"], t0, t1, n, j, j + 1)
            res = self.backprop(work["one"], a, theta, t0, t1, n, j, j + 1)
            if res is not a:
                a.copy_(res)
        return a

    def generic_reverse(self, i, rec):
        yield rec, lambda y: _fixed_torch(self.func, y, self.tl[i - 1], self.tl[i], self.steps[i - 1], self.method)


def _multistep_sweep(fwd, method):
    """(forward_save, backprop, record_floats) of a field under a multistep method - or None."""
    if fwd.multistep_forward_save is None or fwd.multistep_backprop is None:
        return None
    bind = lambda f: (lambda *args, **kw: f(method, *args, **kw))      # noqa: E731
    return bind(fwd.multistep_forward_save), bind(fwd.multistep_backprop), bind(fwd.multistep_record_floats)


class _MultistepBackprop(_Rk4Backprop):
    """What _OdeintBackprop does per interval under a multistep method (K - 1 rk4 start-up steps, then one evaluation per
    step).  Fused (a field offering multistep_forward_save / multistep_backprop: GcnOdeField): a flat record, [y_i, k_1..k_4]
    of a start-up step and [y_i, f_i] of a later one, swept in reverse by one C call per interval - or, when the whole solve
    outgrows BACKPROP_SAVE_MAX_BYTES, y_i alone of the start-up steps, each re-run into a one-step record just before its
    sweep (the later steps' records are kept whole).  An interval of at most K - 1 steps is an rk4 solve and takes
    _Rk4Backprop's path.  Generic: the record is the interval's start state, from which the interval is re-run as torch ops
    through func (_multistep_torch)."""

    def __init__(self, func, fwd, tl, rtol, atol, options, y0c, method):
        self.func, self.fwd, self.tl, self.tols, self.options = func, fwd, tl, (rtol, atol), options
        self.method, self.K, self.S = method, len(MULTISTEP_BETAS[method]), 4
        step_size = (options or {}).get("step_size")
        self.steps = [uniform_grid(tl[i - 1], tl[i], step_size) for i in range(1, len(tl))]
        sweep = _multistep_sweep(fwd, method) if NATIVE_RK4 else None
        rk4 = _fixed_sweep(fwd, "rk4") if NATIVE_RK4 else None
        self.fused = sweep is not None and rk4 is not None
        self.stats = Dopri5Stats()
        self.ms_one = None
        if self.fused:
            self.ms_forward_save, self.ms_backprop, self.floats = sweep
            self.forward_save, self.backprop = rk4                        # _Rk4Backprop's members: the short intervals
            _prepare(fwd)
            nd = y0c.numel()
            total = sum(self.floats(n, n, nd) if n >= self.K else 5 * n * nd for n in self.steps)
            self.save_all = total * 4 <= BACKPROP_SAVE_MAX_BYTES

    def forward(self, i, cur, start):
        n = self.steps[i - 1]
        if not self.fused or n < self.K:
            return _Rk4Backprop.forward(self, i, cur, start)      # generic: _integrate counts; fused: an rk4 interval
        fwd, t0, t1, nd, K = self.fwd, self.tl[i - 1], self.tl[i], cur.numel(), self.K
        like = dict(dtype=cur.dtype, device=cur.device)
        y_end = torch.empty_like(cur)
        if self.save_all:
            rec = torch.empty(self.floats(n, n, nd), **like)
            rec[:nd].copy_(cur.reshape(-1))
            self.ms_forward_save(rec, y_end, rec, t0, t1, n, 0, n)
        else:
            start_n = (K - 1) * nd                                          # y_0 .. y_{K-2}, then the multistep records
            rec = torch.empty(start_n + self.floats(n, n, nd) - self.floats(n, K - 1, nd), **like)
            tmp = torch.empty(self.floats(n, K - 1, nd), **like)           # the start-up records, until the forward is over
            tmp[:nd].copy_(cur.reshape(-1))
            self.ms_forward_save(tmp, rec[start_n:start_n + nd], tmp, t0, t1, n, 0, K - 1)
            for j in range(K - 1):
                rec[j * nd:(j + 1) * nd].copy_(tmp[5 * j * nd:(5 * j + 1) * nd])
            hist = [tmp[(5 * j + 1) * nd:(5 * j + 2) * nd] for j in range(K - 2, -1, -1)]      # k_1 = f of steps K-2 .. 0
            self.ms_forward_save(rec[start_n:start_n + nd], y_end, rec[start_n:], t0, t1, n, K - 1, n, hist=hist)
        self.stats.nfe += _grid_nfe(self.method, n)
        return rec, y_end

    def fused_reverse(self, i, rec, a, theta, work):
        n = self.steps[i - 1]
        if n < self.K:
            return _Rk4Backprop.fused_reverse(self, i, rec, a, theta, work)
        rerun = None
        if not self.save_all:                  # (kept beside `work`, which _Rk4Backprop fills for the short intervals)
            if self.ms_one is None:
                self.ms_one = torch.empty(5 * a.numel(), dtype=a.dtype, device=a.device)
            rerun = self.ms_one
        res = self.ms_backprop(rec, a, theta, self.tl[i - 1], self.tl[i], n, rerun=rerun)
        if res is not a:
            a.copy_(res)
        return a

    def generic_reverse(self, i, rec):
        yield rec, lambda y: _multistep_torch(self.func, y, self.tl[i - 1], self.tl[i], self.steps[i - 1], self.method)


def _adaptive_sweep(fwd, method):
    """(step_native, step_backprop, backprop_work) of a field under an adaptive method, each taking the dopri5 member's
    arguments - None where the field does not offer it.  dopri5 keeps the members it has always used; a field's seven-stage
    dopri5 members never serve another method."""
    if method == "dopri5":
        return fwd.dopri5_step_native, fwd.dopri5_step_backprop, fwd.dopri5_backprop_work
    bind = lambda f: None if f is None else (lambda *args: f(method, *args))      # noqa: E731
    return bind(fwd.adaptive_step_native), bind(fwd.adaptive_step_backprop), bind(fwd.adaptive_backprop_work)


class _Dopri5Backprop:
    """What _OdeintBackprop does per interval under an adaptive method (dopri5, bosh3, adaptive_heun; S stages); the accepted step sizes are constants of the
    derivative.  The forward runs the solve's own launches on buffers a solver.Dopri5Record keeps.  Fused (a field offering
    the method's sweep - _adaptive_sweep: dopri5_step_backprop under dopri5 (GcnOdeField, GatOdeField, qc_ode.EdgeOdeField),
    adaptive_step_backprop under bosh3 / adaptive_heun (GcnOdeField, qc_ode.EdgeOdeField, and GatOdeField with its opt-in
    gat_ode.GatOdeField.ADAPTIVE_NATIVE on - off by default)): y_n and k_1..k_S of every accepted step - or y_n and k_1
    past BACKPROP_SAVE_MAX_BYTES, each step then re-run by one native step call before its sweep (never for a field without
    the method's native step: it keeps all S) - swept in reverse, one call per step (csrc/ode_driver.hip; qc_ode.py).
    Generic: y_n alone, each accepted step re-run as torch ops through func, k_1 = func(t_n, y_n) recomputed: the same
    function of y_n as the derivative FSAL hands over, since Y_S and y_{n+1} are the same combination."""
    own_cotangent = False             # fused_reverse hands back one of its work arrays

    def __init__(self, func, fwd, tl, rtol, atol, options, y0c, method="dopri5"):
        if fwd.fixed_grid_only:
            raise NotImplementedError(_FIXED_ONLY)
        self.func, self.fwd, self.tl, self.tols = func, fwd, tl, (rtol, atol)
        # the other adaptive methods (S stages) go through the adaptive_* members, which take the method first
        self.method, self.S = method, adaptive_stages(method)
        self.step_native, self.step_backprop, self.backprop_work = _adaptive_sweep(fwd, method)
        self.fused = self.step_backprop is not None and solver.DOPRI5_NATIVE
        self.stats = Dopri5Stats()
        self.left = BACKPROP_SAVE_MAX_BYTES
        _prepare(fwd)

    def forward(self, i, cur, start):
        fused, left, S = self.fused, self.left, self.S
        if fused and self.step_native is None:
            rec = Dopri5Record(S, full=S)         # no native step to re-run a step with: all S, whatever the bound
        else:
            rec = Dopri5Record(S, left, full=S) if fused and left is not None else Dopri5Record(1 if fused else 0, full=S)
        (cur,), _ = integrate_adaptive(self.fwd, [cur], self.tl[i - 1], self.tl[i], *self.tols, self.method, self.stats,
                                       record=rec)
        if fused and left is not None:
            self.left = left - rec.bytes if rec.keep == S else None      # past the bound: the later intervals keep k_1 only
        return rec, cur

    def fused_reverse(self, i, rec, a, theta, work):
        S, B = self.S, ADAPTIVE_TABLEAUS[self.method][2]
        if not work:
            # turn: which (ybar_n, kbar_1) pair the next call writes: never the one it reads
            work.update(arrays=self.backprop_work(a), rerun=None, turn=0)
        kbar7 = None
        for j in range(len(rec.steps) - 1, -1, -1):
            t, h, x, y, ks = rec.steps[j]
            ks = [k[0] for k in ks]
            if len(ks) < S:                 # re-run the step into a one-step record (the forward's launches)
                if work["rerun"] is None:
                    work["rerun"] = [torch.empty_like(a) for _ in range(S)]
                rerun = work["rerun"]
                self.step_native(y, [[ks[0]]] + [[b] for b in rerun[:S - 1]], [rerun[S - 1]], t, h, *self.tols)
                ks = [ks[0]] + rerun[:S - 1]
            if x is None:
                wy, wk = 1.0, [h * b for b in B]
            else:
                cy0, cy1, kc = adaptive_interp_weights(self.method, x)
                wy, wk = cy0 + cy1, [h * (cy1 * b + c) for b, c in zip(B, kc)]
            a, kbar7 = self.step_backprop(y[0], ks, a, kbar7, wy, wk, t, h, j == 0, work["arrays"], work["turn"], theta)
            work["turn"] ^= 1
        return a

    def generic_reverse(self, i, rec):
        for (t, h, x, y, _) in reversed(rec.steps):
            yield (_gather(y[0], self.fwd.row_inverse, copy=False),
                   lambda yn, t=t, h=h, x=x: _dopri5_step_torch(self.func, yn, t, h, x, self.method))


class _OdeintBackprop(torch.autograd.Function):
    """odeint with gradients: the forward is odeint's own (bit for bit), the backward the exact derivative of the
    discrete solution.  Per interval of t the method's strategy (_Rk4Backprop / _Dopri5Backprop) supplies
        forward(i, cur, start) -> (record, end state)       cur in the field's row order, start in the caller's,
        fused_reverse(i, record, a, theta, work) -> a       the field's reverse sweep; theta gathers parameter gradients,
        generic_reverse(i, record) -> (y, step) pairs       last piece first: step(y) re-runs a piece as torch ops,
    and this class everything around them."""

    @staticmethod
    def forward(ctx, func, fwd, tl, rtol, atol, method, options, y0, *params):
        y0c = y0.detach().contiguous()
        outs = [y0c.clone()]
        records = []
        with torch.no_grad():
            if method in MULTISTEP_METHODS:
                sweep = _MultistepBackprop(func, fwd, tl, rtol, atol, options, y0c, method)
            elif method in FIXED_METHODS:
                sweep = _Rk4Backprop(func, fwd, tl, rtol, atol, options, y0c, method)
            else:
                sweep = _Dopri5Backprop(func, fwd, tl, rtol, atol, options, y0c, method)
            cur = _gather(y0c, fwd.row_order)
            for i in range(1, len(tl)):
                rec, cur = sweep.forward(i, cur, outs[-1])
                records.append(rec)
                outs.append(_gather(cur, fwd.row_inverse))
        _bump_nfe(func, fwd, sweep.stats.nfe)
        ctx.func, ctx.fwd, ctx.tl, ctx.sweep, ctx.records = func, fwd, tl, sweep, records
        return torch.stack(outs)

    @staticmethod
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous()
        func, fwd, tl, sweep, records = ctx.func, ctx.fwd, ctx.tl, ctx.sweep, ctx.records
        if sweep.fused:
            a = _gather(grad_out[-1], fwd.row_order)
            theta = fwd.packed_grads(a.device)
            work = {}
            with torch.no_grad():
                for i in range(len(tl) - 1, 0, -1):
                    a = sweep.fused_reverse(i, records[i - 1], a, theta, work)
                    if i > 1:
                        a.add_(_gather(grad_out[i - 1], fwd.row_order))
                gy0 = _gather(a, fwd.row_inverse, copy=not sweep.own_cotangent).add_(grad_out[0])
            pg = fwd.packed_param_grads(theta)
        else:
            params = _params(func)
            nfe0 = getattr(func, "nfe", None)
            a = grad_out[-1]
            pg = [None] * len(params)
            for i in range(len(tl) - 1, 0, -1):
                for y_start, step in sweep.generic_reverse(i, records[i - 1]):
                    with torch.enable_grad():
                        y = y_start.detach().requires_grad_(True)
                        g = torch.autograd.grad(step(y), (y,) + tuple(params), a, allow_unused=True)
                    a = g[0] if g[0] is not None else torch.zeros_like(a)
                    for q, gq in enumerate(g[1:]):
                        if gq is not None:
                            pg[q] = gq if pg[q] is None else pg[q] + gq
                a = a + grad_out[i - 1]
            gy0 = a
            if nfe0 is not None:
                func.nfe = nfe0                   # evaluations re-run by the backward pass are not counted (torchdiffeq's
                                                  # odeint counts none in its backward)
        return (None, None, None, None, None, None, None, gy0, *pg)


def odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None):
    """torchdiffeq's odeint.  With grad mode on and y0 or a parameter of func requiring grad the result is differentiable
    (backprop through the solve: _OdeintBackprop; t gets no gradient); otherwise - and always on row-partitioned fields -
    a forward solve without gradient support."""
    _check_state(y0)
    tl = _times(t)
    method = _grid_method(_method(method), tl, options)
    fields = _fields(func, y0)
    fwd = fields[0]
    if torch.is_grad_enabled() and fwd.big_components is None:
        params = _params(func)
        if y0.requires_grad or params:
            covered = tuple(fields[2]) + _extra_inputs(func)       # a field with a sweep returns the extra inputs' gradients too
            same = len(covered) == len(params) and all(p is q for p, q in zip(covered, params))
            if method in MULTISTEP_METHODS:
                sweep = _multistep_sweep(fwd, method)
            else:
                sweep = _fixed_sweep(fwd, method) if method in FIXED_METHODS else _adaptive_sweep(fwd, method)[1]
            if sweep is not None and not same:
                fwd = AutogradField(func, y0)         # the fused field does not cover these parameters
            return _OdeintBackprop.apply(func, fwd, tl, float(rtol), float(atol), method, options, y0, *params)
    stats = Dopri5Stats()
    y0c = y0.detach().contiguous()
    ys = [_gather(y0c, fwd.row_order)]
    outs = [y0c.clone()]
    with torch.no_grad():
        for i in range(1, len(tl)):
            _integrate(fwd, ys, tl[i - 1], tl[i], rtol, atol, method, options, stats)
            outs.append(_gather(ys[0], fwd.row_inverse))
    _bump_nfe(func, fwd, stats.nfe)
    return torch.stack(outs)


class _OdeintAdjoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, func, tl, rtol, atol, method, options, last_only, y0, *params):
        plan, (fwd, mk_adj, plist) = _plan_for(func, y0, tl, method, options, params)
        stats = Dopri5Stats()
        order, inverse = fwd.row_order, fwd.row_inverse
        y0c = y0.detach().contiguous()
        # ans_p[i] = state at tl[i] in the field's row order (what the adjoint starts from); every slice is written in
        # place - the start by the renumbering gather, each later one by the integrator working on that slice - so a
        # solve moves the state through memory twice around the integration instead of once per clone and stack
        # (at 2^20 x 128 a pass is 0.2 ms; the clone-and-stack form made ten of them per forward pass)
        ans_p = torch.empty((len(tl),) + tuple(y0c.shape), dtype=y0c.dtype, device=y0c.device)
        _gather(y0c, order, out=ans_p[0])                       # state rows in the renumbered graph's order
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
        _bump_nfe(func, fwd, stats.nfe)
        ctx.last_only = bool(last_only)
        if last_only:
            # only y(t[-1]) leaves (what the reference's ODEBlock keeps, GCN/models.py:200 `out[1]`): no copy of y0 into
            # a stacked result, and the backward pass gets the cotangent of that one state instead of a zero-filled stack
            ans = _gather(ans_p[-1], inverse)
        elif order is None:
            ans = ans_p
        else:
            ans = torch.empty_like(ans_p)
            ans[0].copy_(y0c)
            for i in range(1, len(tl)):
                _gather(ans_p[i], inverse, out=ans[i])
        ctx.func, ctx.tl, ctx.rtol, ctx.atol, ctx.method, ctx.options = func, tl, rtol, atol, method, options
        ctx.mk_adj = mk_adj
        ctx.fwd = fwd
        ctx.plan = plan
        ctx.rows = (order, inverse)
        ctx.save_for_backward(ans_p)
        return ans

    @staticmethod
    def backward(ctx, grad_out):
        (ans,) = ctx.saved_tensors
        func, tl = ctx.func, ctx.tl
        grad_out = grad_out.contiguous()
        order, inverse = ctx.rows
        back = lambda g: _gather(g, inverse, copy=False)      # noqa: E731
        last_only = ctx.last_only
        n_t = len(tl)

        def g_raw(i):                                 # dL/dy(tl[i]) in the caller's row order, None = zero
            if last_only:
                return grad_out if i in (n_t - 1, -1) else None
            return grad_out[i]

        def g_at(i):                                  # the same in the field's row order (one gather, when asked for)
            g = g_raw(i)
            return None if g is None else _gather(g, order, copy=False)

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
            _bump_nfe(func, plan.adj, plan.gb.nfe, (n_t - 1) if NFE_COUNTS_SKIPPED_DLDT_EVAL else 0)
            return (None, None, None, None, None, None, None, gy0, *plan.adj.param_grads(comps))
        if plan is not None:
            plan.seen_b += 1
        adj = ctx.mk_adj()
        fwd = ctx.fwd
        ctx_tmp = torch.empty_like(ans[0])
        stats = Dopri5Stats()
        with torch.no_grad():
            comps = adj.new_state(ans[-1])
            _gather(g_raw(-1), order, out=comps[1])
            for i in range(len(tl) - 1, 0, -1):
                comps[0].copy_(ans[i])
                if ctx.method not in GRID_METHODS:
                    # dL/dt at the output time enters the adaptive error control (torchdiffeq evaluates
                    # func once more here); a fixed grid never looks at it, so the fixed-grid methods skip the eval.
                    fwd.eval(tl[i], [[(1.0, ans[i])]], [ctx_tmp])
                    stats.nfe += 1
                    gi = g_at(i)
                    if gi is not None:
                        comps[2].sub_((ctx_tmp * gi).sum().reshape(1))
                    if adj.big_components is not None:
                        adj.adaptive = True
                        adj.reduce_small(comps[2])      # row-partitioned: a_t is a sum over all rows
                _integrate(adj, comps, tl[i], tl[i - 1], ctx.rtol, ctx.atol, ctx.method, ctx.options, stats)
                if i > 1 and g_raw(i - 1) is not None:
                    comps[1].add_(g_at(i - 1))
            # the cotangent of the start state is added after the rows are back in the caller's order: one pass, and
            # no gather of a slice that is all zeros whenever the loss only looks at the end state
            gy0 = add_start(back(comps[1]))
        skipped = (n_t - 1) if (ctx.method in GRID_METHODS and NFE_COUNTS_SKIPPED_DLDT_EVAL) else 0
        _bump_nfe(func, adj, stats.nfe, skipped)
        return (None, None, None, None, None, None, None, gy0, *adj.param_grads(comps))


def odeint_adjoint(func, y0, t, rtol=1e-6, atol=1e-12, method=None, options=None, _last_only=False):
    """torchdiffeq's odeint_adjoint for the adaptive methods (dopri5, bosh3, adaptive_heun), the fixed-grid ones (rk4, midpoint, euler)
    and the multistep explicit_adams.  `_last_only=True` (not part of the reference
    API; used by models.ODEBlock, which keeps `out[1]` only) returns y(t[-1]) instead of the stack over t."""
    _check_state(y0)
    tl = _times(t)
    method = _grid_method(_method(method), tl, options)
    if not isinstance(func, torch.nn.Module):
        raise ValueError("odeint_adjoint: func must be an nn.Module")
    params = _params(func)
    return _OdeintAdjoint.apply(func, tl, float(rtol), float(atol), method, options, bool(_last_only), y0, *params)
