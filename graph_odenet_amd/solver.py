"""Own ODE solver behind the torchdiffeq seam of the reference (GCN/models.py:5,192).

torchdiffeq is an un-vendored third-party dependency of the reference; this
module re-creates the two methods the hot path needs from the published algorithms
(see oracle/solver_ref.py for the restatement and its sources):

  * fixed-grid `rk4`  : 3/8-rule steps on a uniform grid (options['step_size']);
  * fixed-grid `euler`, `midpoint` : torchdiffeq's one- and two-stage methods on the same grid, run by the same driver from
                        their tableaus (FIXED_TABLEAUS, integrate_fixed);
  * multistep `explicit_adams` : 4th-order Adams-Bashforth on the same grid, three rk4 start-up steps per interval, then one
                        evaluation per step (MULTISTEP_BETAS, integrate_multistep);
  * adaptive `dopri5` : Dormand-Prince 5(4), FSAL, RMS mixed-tolerance error ratio per
                        state tensor, safety 0.9 / ifactor 10 / dfactor 0.2, 4th-order
                        interpolation to the end time (the reference's default: no
                        `method=` is passed, rtol = atol = 1e-5);
  * adaptive `bosh3`, `adaptive_heun` : Bogacki-Shampine 3(2) and Heun-Euler 2(1) in FSAL form, run by the same driver as
                        dopri5 from their tableaus (ADAPTIVE_TABLEAUS, integrate_adaptive): the controller with exponent
                        1/p, the cubic Hermite fit at the end time;
  * `odeint_adjoint`  : O(1)-memory adjoint; the augmented state (y, a, [a_t], a_theta) is
                        integrated backwards with the same method.

All state arithmetic (stage inputs, solution combine, error ratio, interpolation) runs in
the HIP kernels of csrc/rk.hip through `ops`; the vector field is a "field" object that
consumes stage inputs as (coef, tensor) term lists so that a fused field (gcn_ode.py) never
materialises them.  Step acceptance is host logic (one device->host sync per adaptive step).
"""
import math

import torch

from . import ops

# 3/8-rule (Kutta 1901): c = [0, 1/3, 2/3, 1]
RK38_C = [0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0]
RK38_A = [[], [1.0 / 3.0], [-1.0 / 3.0, 1.0], [1.0, -1.0, 1.0]]
RK38_B = [1.0 / 8.0, 3.0 / 8.0, 3.0 / 8.0, 1.0 / 8.0]

# explicit Euler, and the explicit midpoint rule as torchdiffeq states it (b_1 = 0: the result never reads k_1)
EULER_C, EULER_A, EULER_B = [0.0], [[]], [1.0]
MIDPOINT_C, MIDPOINT_A, MIDPOINT_B = [0.0, 0.5], [[], [0.5]], [0.0, 1.0]
# the fixed-grid methods by name: (c, a, b); the order is that of the GODE_RK_* codes of include/graphode.h
FIXED_TABLEAUS = {"rk4": (RK38_C, RK38_A, RK38_B), "euler": (EULER_C, EULER_A, EULER_B),
                  "midpoint": (MIDPOINT_C, MIDPOINT_A, MIDPOINT_B)}
FIXED_METHODS = tuple(FIXED_TABLEAUS)


# The multistep methods by name: the weights beta_j of f_{i-j} in  y_{i+1} = y_i + h sum_j beta_j f_{i-j}.  explicit_adams is the
# 4th-order Adams-Bashforth method on the fixed grid, started with len(beta) - 1 3/8-rule steps whose k_1 = f_i is kept
# (integrate_multistep); the history restarts at every interval of t.  They have no GODE_RK_* code: include/graphode.h gives
# them entry points of their own (gode_gcn_ode_adams_*).
ADAMS_BETA = [55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0]
MULTISTEP_BETAS = {"explicit_adams": ADAMS_BETA}
MULTISTEP_METHODS = ("explicit_adams",)


def multistep_nfe(method, n):
    """Evaluations of an n-step solve of one interval: four per start-up step, one per multistep step."""
    start = min(n, len(MULTISTEP_BETAS[method]) - 1)
    return 4 * start + (n - start)


def multistep_weight(method, i, n, h):
    """The weight f_i (the evaluation that opens step i of n) ends up with over all multistep steps that read it:
    h * sum of beta_{m - i} over the steps m = max(i, K - 1) .. min(i + K - 1, n - 1), formed in double.  A component no
    stage input reads (a pure quadrature) may take each evaluation once with this weight instead of keeping a history."""
    beta = MULTISTEP_BETAS[method]
    K = len(beta)
    return h * sum(beta[m - i] for m in range(max(i, K - 1), min(i + K - 1, n - 1) + 1))


def method_code(method):
    """The GODE_RK_* code of a fixed-grid method name."""
    return FIXED_METHODS.index(method)


def n_stages(method):
    return len(FIXED_TABLEAUS[method][0])


DP_C = [0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0]
DP_A = [
    [],
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
    [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
]
DP_B = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
DP_E = [
    35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720,
    -2187 / 6784 - -12231 / 42400, 11 / 84 - 649 / 6300, -1.0 / 60.0,
]
DP_MID = [
    6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
    187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2,
]


def interp_weights(x):
    """(cy0, cy1, kc[7]): the 4th-order fit through (y_n, y_mid, y_{n+1}, f_n, f_{n+1}) of a step at abscissa x, as
    cy0 y_n + cy1 y_{n+1} + h sum kc_s k_s."""
    x2, x3, x4 = x * x, x * x * x, x * x * x * x
    wm = 16 * x4 - 32 * x3 + 16 * x2
    cy0 = -8 * x4 + 18 * x3 - 11 * x2 + 1 + wm
    cy1 = -8 * x4 + 14 * x3 - 5 * x2
    kc = [wm * m for m in DP_MID]
    kc[0] += -2 * x4 + 5 * x3 - 4 * x2 + x
    kc[6] += 2 * x4 - 3 * x3 + x2
    return cy0, cy1, kc


# Bogacki-Shampine 3(2) and Heun-Euler 2(1), both written in FSAL form as Dormand-Prince is: the last row of a equals b, so
# k_S of an accepted step is k_1 of the next.  Heun-Euler's natural two-stage form is not FSAL; its third stage f(t + h, y1)
# makes it so, at the price of one wasted evaluation per rejected attempt.  e = b - b*.
BS_C = [0.0, 1 / 2, 3 / 4, 1.0]
BS_A = [[], [1 / 2], [0, 3 / 4], [2 / 9, 1 / 3, 4 / 9]]
BS_B = [2 / 9, 1 / 3, 4 / 9, 0]
BS_E = [2 / 9 - 7 / 24, 1 / 3 - 1 / 4, 4 / 9 - 1 / 3, -1 / 8]
HE_C = [0.0, 1.0, 1.0]
HE_A = [[], [1.0], [1 / 2, 1 / 2]]
HE_B = [1 / 2, 1 / 2, 0]
HE_E = [-1 / 2, 1 / 2, 0]
# the adaptive methods by name: (c, a, b, e, order p); the order is that of the GODE_RKA_* codes of include/graphode.h
ADAPTIVE_TABLEAUS = {"dopri5": (DP_C, DP_A, DP_B, DP_E, 5), "bosh3": (BS_C, BS_A, BS_B, BS_E, 3),
                     "adaptive_heun": (HE_C, HE_A, HE_B, HE_E, 2)}
ADAPTIVE_METHODS = tuple(ADAPTIVE_TABLEAUS)


def adaptive_code(method):
    """The GODE_RKA_* code of an adaptive method name."""
    return ADAPTIVE_METHODS.index(method)


def adaptive_stages(method):
    return len(ADAPTIVE_TABLEAUS[method][0])


def hermite_weights(x, S):
    """(cy0, cy1, kc[S]): the cubic Hermite fit through (y_n, f_n, y_{n+1}, f_{n+1}) of an FSAL-form step at abscissa x, in
    interp_weights' form (f_n = k_1, f_{n+1} = k_S)."""
    x2, x3 = x * x, x * x * x
    kc = [0.0] * S
    kc[0] = x3 - 2 * x2 + x
    kc[S - 1] = x3 - x2
    return 2 * x3 - 3 * x2 + 1, -2 * x3 + 3 * x2, kc


def adaptive_interp_weights(method, x):
    """The end-of-interval fit of an adaptive method: dopri5's quartic (interp_weights), the cubic Hermite fit otherwise."""
    return interp_weights(x) if method == "dopri5" else hermite_weights(x, adaptive_stages(method))


class Field:
    """A vector field over a list of state components.

    eval(t, terms, out): terms[c] is the (coef, tensor) list whose sum is the stage value of
    component c; out[c] receives d(component c)/dt.  t is a python float.

    Everything below `eval` is optional and states the whole protocol between the fields and the two solver modules:
    a field offers a member by overriding it, and None / False / () means "absent" (the solvers then take the plain path).
    """
    n_components = 1

    def eval(self, t, terms, out):   # pragma: no cover - interface
        raise NotImplementedError

    # ---- both integrators -----------------------------------------------------------------------------------------
    prepare = None                # prepare(): odeint, once before a solve issues launches (refresh packed parameters)
    alloc_like = None             # alloc_like(y, n) -> n work copies of the state y: both integrators, at their start
    fused = False                 # the field never calls func.forward: odeint adds the solve's nfe to func.nfe itself
    row_order = None              # the field integrates y[row_order] (models.ODEfunc marks it): odeint gathers on entry
    row_inverse = None            # ... and gathers with row_inverse on exit
    token = None                  # identity of the problem besides shapes and parameters (what func.gode_plan_token gives)
    # ---- fixed-grid rk4 -------------------------------------------------------------------------------------------
    rk4_native = None             # rk4_native(comps, t0, t1, n) -> nfe: odeint, the whole solve as one C call
    eval_combine = None           # eval_combine(t, terms, pre, coef, out) -> components whose new solution it wrote to
    #                               out: integrate_rk4, instead of eval for the last stage of a step
    begin_rk4_step = None         # begin_rk4_step() -> bool: integrate_rk4 before the stages of a step; True = this step's
    finish_rk4_step = None        # ... deferred_components are advanced in place by finish_rk4_step(weights, y) after them
    deferred_components = ()
    fixed_grid_only = False       # odeint refuses the adaptive method on this field
    # ---- every fixed-grid method (a name of FIXED_TABLEAUS; S stages) ---------------------------------------------------
    #                               eval_combine / begin_rk4_step / finish_rk4_step serve integrate_fixed as they serve
    #                               integrate_rk4: the last stage closes the step, finish_rk4_step receives S weights
    fixed_native = None           # fixed_native(comps, t0, t1, n, method) -> nfe: odeint, the whole solve as one C call;
    #                               None from the call itself = not on this route, take the per-stage driver
    # ---- the multistep methods (a name of MULTISTEP_BETAS) on more steps than the start-up takes -------------------------------
    #                               begin_rk4_step / finish_rk4_step serve integrate_multistep too: a multistep step is one
    #                               evaluation, and finish_rk4_step receives each evaluation's final weight (multistep_weight)
    multistep_native = None       # multistep_native(comps, t0, t1, n, method) -> nfe: odeint, the whole solve as one C call;
    #                               None from the call itself = not on this route, take integrate_multistep
    multistep_forward_save = None  # multistep_forward_save(method, y0, y_end, save, t0, t1, n, i0, i1, hist=None): steps i0..i1-1
    #                               into the flat record `save` - [y_i, k_1..k_4] of a start-up step, [y_i, f_i] of a later
    #                               one; multistep_record_floats(method, n, step, nd) -> the floats in front of step's record
    multistep_record_floats = None
    multistep_backprop = None     # multistep_backprop(method, save, a, theta, t0, t1, n, rerun=None) -> tensor holding dL/dy
    #                               before step 0; rerun: a one-step rk4 record, `save` then keeps y_i alone of the start-up
    # ---- adaptive dopri5 ------------------------------------------------------------------------------------------
    dopri5_step_native = None     # dopri5_step_native(y, kk, y1, t, h, rtol, atol) -> error sums per ratio group (fp64,
    #                               on the device): integrate_dopri5, one attempted step as one C call
    ratio_groups = None           # components whose error norms pool (a state tensor of torchdiffeq): both error norms
    # ---- the other adaptive methods (a name of ADAPTIVE_TABLEAUS; S stages) ---------------------------------------------------
    #                               the dopri5_* members keep their meaning and serve dopri5 alone; a field without the
    #                               members below runs these methods on the per-stage driver through `eval` (the GCN fields
    #                               offer the step, the GAT fields with gat_ode.GatOdeField.ADAPTIVE_NATIVE on - off by
    #                               default; they and qc_ode.EdgeOdeField the sweep further down)
    adaptive_step_native = None   # adaptive_step_native(method, y, kk, y1, t, h, rtol, atol) -> error sums per ratio group:
    #                               integrate_adaptive, one attempted step (kk: S stage buffers) as one C call
    # ---- row-partitioned fields (big_components is not None) ------------------------------------------------------------
    big_components = None         # the components that are row slices; odeint keeps such fields forward-only
    adaptive = False              # set by odeint before an adaptive solve: the small components are then kept global
    global_numel = None           # global_numel(c, t) -> elements of component c over all ranks: the error norms
    reduce_error_sums = None      # reduce_error_sums(sums) -> the per-component sums over all ranks: the error norms
    reduce_small = None           # reduce_small(t): sum a small component over the ranks in place (adjoint, adaptive)
    # ---- adjoint fields (odeint._OdeintAdjoint.backward) ---------------------------------------------------------------
    new_state = None              # new_state(y_end) -> [y, a = 0, a_t = 0, parameter gradients = 0 ...]
    param_grads = None            # param_grads(comps) -> the gradients in func.parameters() order (+ extra inputs)
    # ---- backprop through the solve (odeint._OdeintBackprop); a field offering a sweep offers the packed pair too ----------
    rk4_forward_save = None       # rk4_forward_save(y0, y_end, save, t0, t1, n, i0, i1): steps i0..i1-1, stages recorded
    rk4_backprop = None           # rk4_backprop(save, a, theta, t0, t1, n, i0, i1) -> tensor holding dL/dy before step i0
    fixed_forward_save = None     # fixed_forward_save(method, y0, y_end, save, t0, t1, n, i0, i1): the same for any fixed-grid
    #                               method; a step's record is [y_n, k_1..k_S]
    fixed_backprop = None         # fixed_backprop(method, save, a, theta, t0, t1, n, i0, i1) -> as rk4_backprop
    dopri5_step_backprop = None   # dopri5_step_backprop(y, k, g, kbar7, wy, wk, t, h, first, work, turn, theta); a field
    #                               offering it without dopri5_step_native gets all seven k_s of every step, whatever the
    #                               byte bound (there is nothing to re-run a step with)
    dopri5_backprop_work = None   # dopri5_backprop_work(like) -> the work arrays dopri5_step_backprop takes
    adaptive_step_backprop = None  # adaptive_step_backprop(method, y, k, g, kbar_last, wy, wk, t, h, first, work, turn, theta):
    #                               dopri5_step_backprop for the other adaptive methods (k, wk of S entries)
    adaptive_backprop_work = None  # adaptive_backprop_work(method, like) -> the work arrays adaptive_step_backprop takes
    packed_grads = None           # packed_grads(device) -> zeroed buffer `theta` the sweeps add parameter gradients to
    packed_param_grads = None     # packed_param_grads(theta) -> the gradients in func.parameters() order


def _stage_terms(y, ks, coefs, h):
    """terms of  y + h * sum_j coefs[j] * ks[j]  per component (zero coefficients dropped)."""
    nc = len(y)
    out = []
    for c in range(nc):
        tl = [(1.0, y[c])]
        for j, a in enumerate(coefs):
            if a != 0.0:
                tl.append((h * a, ks[j][c]))
        out.append(tl)
    return out


def _alloc_like(y, n):
    return [[torch.empty_like(c) for c in y] for _ in range(n)]


def uniform_grid(t0, t1, step_size):
    """Number of equal steps covering [t0, t1] with |h| <= step_size (last step not shortened:
    the grid is re-spaced uniformly, which coincides with torchdiffeq's grid whenever
    (t1-t0)/step_size is an integer, e.g. 1/16 on [0,1])."""
    if step_size is None:
        return 1
    n = int(math.ceil(abs(t1 - t0) / step_size - 1e-9))
    return max(n, 1)


def integrate_rk4(field, y, t0, t1, n_steps, work=None):
    """3/8-rule integration of the component list y from t0 to t1.  Returns nfe.

    The entries of the list `y` hold the result on return; they may have been re-bound to other
    buffers (a fused field writes y + h*sum(b_i k_i) straight from the launch that produces the last
    stage and the solution / stage buffers swap roles), so callers read `y[c]` afterwards."""
    # a field may lay out the work copies itself (the adjoint field packs its small components into one buffer, which
    # the fused launch-bound stage writes in one launch)
    alloc = field.alloc_like or _alloc_like
    ks = work if work is not None else alloc(y, 4)
    h = (t1 - t0) / n_steps
    nfe = 0
    nc = len(y)
    fused = field.eval_combine
    # a field may keep the stage derivatives of its SMALL components (a_t, parameter gradients: the adjoint ODE is linear
    # in them and no stage input reads them) as block partials and close the four stages of a step with ONE launch that
    # adds h * sum_s b_s k_s to the solution (gat_ode, one head or H, on launch-bound graphs): begin_rk4_step() before the
    # stages, finish_rk4_step(weights, y) after them returns the components it has advanced
    begin, finish = field.begin_rk4_step, field.finish_rk4_step
    for i in range(n_steps):
        t = t0 + i * h
        deferred = begin is not None and begin()
        for s in range(3):
            field.eval(t + RK38_C[s] * h, _stage_terms(y, ks, RK38_A[s], h), ks[s])
        done = ()
        if fused is not None:
            pre = [[(1.0, y[c])] + [(h * RK38_B[s], ks[s][c]) for s in range(3)] for c in range(nc)]
            done = fused(t + RK38_C[3] * h, _stage_terms(y, ks, RK38_A[3], h), pre, h * RK38_B[3], ks[3])
        else:
            field.eval(t + RK38_C[3] * h, _stage_terms(y, ks, RK38_A[3], h), ks[3])
        nfe += 4
        if deferred:
            done = tuple(done) + tuple(finish([h * b for b in RK38_B], y))
        todo = []
        for c in range(nc):
            if c in done:
                if deferred and c in field.deferred_components:
                    continue                           # advanced in place by finish_rk4_step
                y[c], ks[3][c] = ks[3][c], y[c]        # ks[3][c] already holds the new solution
            else:
                todo.append(c)
        # the remaining components in one launch per group of four (an adjoint state has four: one launch instead of four)
        for g0 in range(0, len(todo), 4):
            grp = todo[g0:g0 + 4]
            terms = [[(1.0, y[c])] + [(h * RK38_B[s], ks[s][c]) for s in range(4)] for c in grp]
            if len(grp) == 1:
                ops.lincomb_(y[grp[0]], terms[0])
            else:
                ops.lincomb_multi_([y[c] for c in grp], terms)
    return nfe


def _fixed_step(field, y, ks, t, h, tableau, extra=None):
    """One step of a fixed-grid method from the component list y at time t (integrate_fixed's body).  extra: a weight added
    to k_1's in finish_rk4_step (the deferred components of a multistep start-up step); no other launch sees it."""
    C, A, B = tableau
    S = len(C)
    L = S - 1
    nc = len(y)
    fused = field.eval_combine
    begin, finish = field.begin_rk4_step, field.finish_rk4_step
    deferred = begin is not None and begin()
    for s in range(L):
        field.eval(t + C[s] * h, _stage_terms(y, ks, A[s], h), ks[s])
    done = ()
    if fused is not None:
        pre = [[(1.0, y[c])] + [(h * B[s], ks[s][c]) for s in range(L) if B[s] != 0.0] for c in range(nc)]
        done = fused(t + C[L] * h, _stage_terms(y, ks, A[L], h), pre, h * B[L], ks[L])
    else:
        field.eval(t + C[L] * h, _stage_terms(y, ks, A[L], h), ks[L])
    if deferred:
        weights = [h * b for b in B]
        if extra is not None:
            weights[0] += extra
        done = tuple(done) + tuple(finish(weights, y))
    todo = []
    for c in range(nc):
        if c in done:
            if deferred and c in field.deferred_components:
                continue                           # advanced in place by finish_rk4_step
            y[c], ks[L][c] = ks[L][c], y[c]        # ks[L][c] already holds the new solution
        else:
            todo.append(c)
    for g0 in range(0, len(todo), 4):
        grp = todo[g0:g0 + 4]
        terms = [[(1.0, y[c])] + [(h * B[s], ks[s][c]) for s in range(S) if B[s] != 0.0] for c in grp]
        if len(grp) == 1:
            ops.lincomb_(y[grp[0]], terms[0])
        else:
            ops.lincomb_multi_([y[c] for c in grp], terms)
    return deferred


def integrate_fixed(field, y, t0, t1, n_steps, method, work=None):
    """integrate_rk4 for any method of FIXED_TABLEAUS, the same protocol: `eval` for every stage but the last,
    `eval_combine` for the last - its pre is y + h * sum of the earlier stages with a non-zero b, its coefficient h * b_last -
    begin_rk4_step / finish_rk4_step around the stages (S weights), and the remaining components in lincomb_multi_ launches of
    four.  Terms with a zero coefficient are dropped.  Returns nfe; read the result from `y[c]`."""
    tableau = FIXED_TABLEAUS[method]
    S = len(tableau[0])
    alloc = field.alloc_like or _alloc_like
    ks = work if work is not None else alloc(y, S)
    h = (t1 - t0) / n_steps
    for i in range(n_steps):
        _fixed_step(field, y, ks, t0 + i * h, h, tableau)
    return S * n_steps


def integrate_multistep(field, y, t0, t1, n_steps, method, work=None):
    """A method of MULTISTEP_BETAS (K weights) on n_steps equal steps from t0 to t1, the protocol of integrate_fixed.  Steps
    0 .. min(n_steps, K - 1) - 1 are integrate_fixed's rk4 step (eval_combine and the deferral honoured); their k_1 = f_i is
    kept.  A later step is one `eval` of f_i on y_i, then  y += h sum_j beta_j f_{i-j}  over the components in lincomb_multi_
    launches of four (K + 1 terms; eval_combine is not used there: it would not leave f_i for the steps after it).  Where the
    field defers components (begin_rk4_step), no history of theirs exists: finish_rk4_step adds each evaluation once with the
    weight it ends up with (multistep_weight; a start-up step's k_1 gets it on top of h b_1), so such a component holds its
    value at t1 only when the solve is over.  work: K + 2 work copies of the state.  Returns nfe; read the result from `y[c]`."""
    beta = MULTISTEP_BETAS[method]
    K = len(beta)
    if n_steps < K:                                     # start-up only: the rk4 solve itself
        return integrate_fixed(field, y, t0, t1, n_steps, "rk4", work[:4] if work is not None else None)
    alloc = field.alloc_like or _alloc_like
    bufs = list(work) if work is not None else alloc(y, K + 2)
    ks, spare = bufs[:4], bufs[4:]
    h = (t1 - t0) / n_steps
    nc = len(y)
    hist = []                                           # f_{i-1}, f_{i-2}, ... (newest first)
    begin, finish = field.begin_rk4_step, field.finish_rk4_step
    for i in range(K - 1):
        _fixed_step(field, y, ks, t0 + i * h, h, FIXED_TABLEAUS["rk4"], extra=multistep_weight(method, i, n_steps, h))
        hist.insert(0, ks[0])
        ks[0] = spare.pop() if spare else ks[1]         # after the last start-up step ks is free: its buffers go on as the ring
    free = [b for b in ks if all(b is not q for q in hist)][:1]
    for i in range(K - 1, n_steps):
        t = t0 + i * h
        fnew = free.pop() if free else hist.pop()       # the buffer of f_{i-K}, which no later step reads
        deferred = begin is not None and begin()
        field.eval(t, [[(1.0, y[c])] for c in range(nc)], fnew)
        hist.insert(0, fnew)
        done = tuple(finish([multistep_weight(method, i, n_steps, h)], y)) if deferred else ()
        todo = [c for c in range(nc) if c not in done]
        for g0 in range(0, len(todo), 4):
            grp = todo[g0:g0 + 4]
            terms = [[(1.0, y[c])] + [(h * beta[j], hist[j][c]) for j in range(K)] for c in grp]
            if len(grp) == 1:
                ops.lincomb_(y[grp[0]], terms[0])
            else:
                ops.lincomb_multi_([y[c] for c in grp], terms)
    return multistep_nfe(method, n_steps)


DOPRI5_NATIVE = True      # fused fields: one C-ABI call per adaptive step (False: per-stage Python driver)


class Dopri5Stats:
    def __init__(self):
        self.accepted = 0
        self.rejected = 0
        self.nfe = 0
        self.attempts = []          # (|dt|, accepted) of every attempted step, in order


# Test hooks.  TRACE: when a list, every adaptive solve appends its attempt sequence [(|dt|, accepted, error ratio), ...]
# to it (forward solve first, then the adjoint solve) - the tests compare it with the oracle solver's sequence.
# REPLAY: when a list of such sequences, the solves consume them in order and take THOSE step sizes and decisions
# instead of the controller's (the oracle's discretisation on the product's kernels: arithmetic parity of the steps
# themselves, independent of accept / reject ties that fp32 rounding decides either way).
TRACE = None
REPLAY = None


def _numel(field, y, c):
    """Elements of component c in the WHOLE problem (a row-partitioned field holds a slice of the big components)."""
    return field.global_numel(c, y[c]) if field.global_numel is not None else y[c].numel()


# Norm of the initial-step heuristic (Hairer-Norsett-Wanner II.4) on a state of several tensors - the adjoint solve's
# (y, a, a_t, a_theta); a one-tensor forward solve is the same either way:
#   "per_tensor" (default): d0, d1, d2 are formed per state tensor (RMS each) and combined as
#                 h0 = 0.01 * max_i(d0_i / d1_i),  h1 = (0.01 / max_i(d1_i, d2_i))^(1/5),  guards on max_i d0_i, max_i d1_i -
#                 the form torchdiffeq 0.0.x (the reference's era) is publicly understood to use, and consistent with
#                 its per-tensor error ratio; NOT checkable here (torchdiffeq is absent: oracle/solver_ref.py);
#   "pooled":     one RMS over all elements of all tensors (rounds 1-2 of this build; what a single flat state gives).
# The two differ in the FIRST attempted step of an adjoint solve only (tests/test_solver_oracle.py shows a 4-tensor
# state where they do); every later step is set by the controller from per-tensor error ratios in both.
INITIAL_STEP_NORM = "per_tensor"


def _div(a, b):
    if b == 0.0:
        return float("nan") if a == 0.0 else float("inf")
    return a / b


def _rms_groups(terms_per_comp, y, rtol, atol, field, pooled):
    """RMS of v / (atol + rtol*|y|) per ratio group (per state tensor as torchdiffeq sees it), or one pooled value.
    -> list of python floats (one device->host sync)."""
    nc = len(y)
    outs = [ops.rk_scaled_sumsq(terms_per_comp[c], y[c], rtol, atol) for c in range(nc)]
    sums = torch.cat(outs).tolist()
    if field.reduce_error_sums is not None:
        sums = field.reduce_error_sums(sums)
    groups = [list(range(nc))] if pooled else (field.ratio_groups or [[c] for c in range(nc)])
    return [math.sqrt(sum(sums[c] for c in grp) / sum(_numel(field, y, c) for c in grp)) for grp in groups]


def _initial_step(field, t0, y, f0, rtol, atol, sgn, scratch_y, scratch_f, stats, order=5):
    if INITIAL_STEP_NORM not in ("per_tensor", "pooled"):
        raise ValueError("solver.INITIAL_STEP_NORM must be 'per_tensor' or 'pooled'")
    pooled = INITIAL_STEP_NORM == "pooled"
    nc = len(y)
    d0 = _rms_groups([[(1.0, y[c])] for c in range(nc)], y, rtol, atol, field, pooled)
    d1 = _rms_groups([[(1.0, f0[c])] for c in range(nc)], y, rtol, atol, field, pooled)
    if max(d0) < 1e-5 or max(d1) < 1e-5:
        h0 = 1e-6
    else:
        h0 = 0.01 * max(_div(a, b) for a, b in zip(d0, d1))
    field.eval(t0 + sgn * h0, [[(1.0, y[c]), (sgn * h0, f0[c])] for c in range(nc)], scratch_f)
    stats.nfe += 1
    d2 = [v / h0 for v in _rms_groups([[(1.0, scratch_f[c]), (-1.0, f0[c])] for c in range(nc)], y, rtol, atol, field,
                                      pooled)]
    if max(d1) <= 1e-15 and max(d2) <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1 + d2)) ** (1.0 / order)
    return min(100 * h0, h1)


def _optimal_step(last, ratio, safety=0.9, ifactor=10.0, dfactor=0.2, order=5):
    if ratio == 0:
        return last * ifactor
    if ratio < 1:
        dfactor = 1.0
    er = math.sqrt(ratio)
    factor = max(1.0 / ifactor, min(er ** (1.0 / order) / safety, 1.0 / dfactor))
    return last / factor


class Dopri5Record:
    """What backprop through an adaptive solve keeps of it (odeint._OdeintBackprop under dopri5): one entry per accepted step,
    (t_n, h_n, x, y_n, [k_1..k_keep]) with x the interpolation abscissa of a last step that overshot the end time, else
    None.  keep = S (7 under dopri5): all stage derivatives; 1: k_1 only; 0: the state alone.  The entries hold the solve's
    own buffers, which the solve then leaves alone; with max_bytes given, a record of `full` = S that outgrows it drops to 1."""

    def __init__(self, keep, max_bytes=None, full=7):
        self.keep, self.max_bytes, self.full = keep, max_bytes, full
        self.steps = []
        self.bytes = 0

    def accepted(self, t, h, x, y, kk):
        """-> how many of the leading stage buffers kk[0..] the record has kept."""
        self.steps.append((t, h, x, y, list(kk[:self.keep])))
        self.bytes += sum(c.numel() * c.element_size() for c in y) * (1 + self.keep)
        if self.keep == self.full and self.keep > 1 and self.max_bytes is not None and self.bytes > self.max_bytes:
            self.keep = 1
            self.steps = [(t_, h_, x_, y_, k_[:1]) for (t_, h_, x_, y_, k_) in self.steps]
        return self.keep


def integrate_adaptive(field, y, t0, t1, rtol, atol, method="dopri5", stats=None, max_steps=100000, record=None):
    """In-place adaptive integration of the component list y from t0 to t1 (either direction) by a method of
    ADAPTIVE_TABLEAUS.  record (a Dopri5Record): every accepted step is entered there with the buffers that hold its y_n and
    stage derivatives, and the solve continues in fresh ones (a rejected attempt's are reused) - the same launches on other
    addresses, so the values are bit for bit those of the plain solve; the result is then returned in a buffer of its own.
    dopri5 takes the launches it has always taken; the other methods close an attempt with ops.rk_close_err_multi."""
    C, A, B, E, p = ADAPTIVE_TABLEAUS[method]
    S = len(C)
    dp = method == "dopri5"
    stats = stats if stats is not None else Dopri5Stats()
    nc = len(y)
    sgn = 1.0 if t1 >= t0 else -1.0
    span = abs(t1 - t0)
    # a field may lay out the work copies of the state itself (e.g. small components packed in one buffer) and may
    # offer the whole step as one native call (csrc/ode_driver.hip) when `dopri5_native` is set
    alloc = field.alloc_like or _alloc_like
    native = None
    if DOPRI5_NATIVE:
        native = field.dopri5_step_native if dp else field.adaptive_step_native
        if native is not None and not dp:
            native = (lambda f: lambda *args: f(method, *args))(native)
    ks = alloc(y, S)
    y1, tmp = alloc(y, 2)
    field.eval(t0, [[(1.0, y[c])] for c in range(nc)], ks[0])
    stats.nfe += 1
    dt = _initial_step(field, t0, y, ks[0], rtol, atol, sgn, tmp, y1, stats, p)
    seq = []                       # (|dt|, accepted, ratio) of every attempt of THIS solve
    forced = REPLAY.pop(0) if REPLAY else None
    if forced is not None:
        dt = float(forced[0][0])
    tau = 0.0                      # elapsed |t - t0|
    fsal = 0                       # index of the buffer that currently holds f(t, y)
    last = None
    steps = 0
    while tau < span:
        steps += 1
        if steps > max_steps:
            raise RuntimeError("%s: max_num_steps exceeded" % method)
        h = sgn * dt
        # stage buffers: slot 0 is whichever buffer holds the FSAL value
        order = [fsal] + [i for i in range(S) if i != fsal]
        kk = [ks[i] for i in order]
        t = t0 + sgn * tau
        groups = field.ratio_groups or [[c] for c in range(nc)]
        if native is not None:
            gsums = native(y, kk, y1, t, h, rtol, atol).tolist()     # one call, one device->host sync
            stats.nfe += S - 1
            ratios = [gs / sum(y[c].numel() for c in grp) for gs, grp in zip(gsums, groups)]
        else:
            for s in range(1, S):
                field.eval(t + C[s] * h, _stage_terms(y, kk, A[s], h), kk[s])
                stats.nfe += 1
            if dp:
                for c in range(nc):
                    ops.lincomb_(y1[c], [(1.0, y[c])] + [(h * B[s], kk[s][c]) for s in range(S) if B[s] != 0.0])
                sums = [ops.rk_error_sumsq(y[c], y1[c], [(h * E[s], kk[s][c]) for s in range(S) if E[s] != 0.0],
                                           rtol, atol) for c in range(nc)]
            else:
                # solution and error sums from one pass over the stages, four components per pair of launches
                live = [s for s in range(S) if B[s] != 0.0 or E[s] != 0.0]
                ec = [0.0] + [h * E[s] for s in live]
                sums = [ops.rk_close_err_multi(y1[c0:c0 + 4],
                                               [[(1.0, y[c])] + [(h * B[s], kk[s][c]) for s in live]
                                                for c in range(c0, min(c0 + 4, nc))],
                                               [ec] * (min(c0 + 4, nc) - c0), rtol, atol) for c0 in range(0, nc, 4)]
            sums = torch.cat(sums).tolist()          # the one device->host sync of this step
            if field.reduce_error_sums is not None:
                sums = field.reduce_error_sums(sums)     # row-partitioned state: every rank sees the global sums
            ratios = [sum(sums[c] for c in grp) / sum(_numel(field, y, c) for c in grp) for grp in groups]
        ratio = max(ratios)
        accept = all(r <= 1.0 for r in ratios) if forced is None else bool(forced[len(seq)][1])
        seq.append((dt, accept, ratio))
        if accept:
            stats.accepted += 1
            if tau + dt >= span:
                # interpolate back to the end time: dopri5's 4th-order fit through (y0, y_mid, y1, f0, f1), the cubic
                # Hermite fit through (y0, f0, y1, f1) for the other methods
                x = (span - tau) / dt
                res = y                                   # the result overwrites y_n, unless a record keeps that
                if record is not None:
                    record.accepted(t, h, x if x < 1.0 else None, y, kk)
                    res = y1 if x >= 1.0 else alloc(y, 1)[0]
                if x >= 1.0:
                    for c in range(nc):
                        if res[c] is not y1[c]:
                            res[c].copy_(y1[c])
                else:
                    cy0, cy1, kc = adaptive_interp_weights(method, x)
                    for c in range(nc):
                        ops.lincomb_(res[c], [(cy0, y[c]), (cy1, y1[c])] +
                                     [(h * kc[s], kk[s][c]) for s in range(S) if kc[s] != 0.0])
                y = res
                tau = span
                break
            if record is not None:
                kept = record.accepted(t, h, None, y, kk)
                for j in range(min(kept, S - 1)):         # kk[S - 1] goes on as the next step's k_1 and is read only
                    ks[order[j]] = alloc(y, 1)[0]
                y = alloc(y, 1)[0]                        # takes y1's place below
            y, y1 = y1, y
            last = y1
            tau += dt
            fsal = order[S - 1]
        else:
            stats.rejected += 1
        dt = _optimal_step(dt, ratio, order=p) if forced is None else float(forced[min(len(seq), len(forced) - 1)][0])
    stats.attempts.extend(seq)
    if TRACE is not None:
        TRACE.append(seq)
    return y, stats


def integrate_dopri5(field, y, t0, t1, rtol, atol, stats=None, max_steps=100000, record=None):
    """integrate_adaptive under Dormand-Prince 5(4)."""
    return integrate_adaptive(field, y, t0, t1, rtol, atol, "dopri5", stats, max_steps, record)


def integrate_dopri5_inplace(field, y, t0, t1, rtol, atol, stats=None, method="dopri5"):
    """Wrapper keeping the caller's tensors as the result holders."""
    res, stats = integrate_adaptive(field, list(y), t0, t1, rtol, atol, method, stats)
    for dst, src in zip(y, res):
        if dst.data_ptr() != src.data_ptr():
            dst.copy_(src)
    return stats
