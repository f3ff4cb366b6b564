"""explicit_adams restated for the tests, in the manner of tests/fixed_methods_ref.py (whose yardstick, graphs and reference
functions are imported, not copied): plain loops in whatever dtype the state has, for any callable func(t, y) -> dy/dt.

The method on one interval [t0, t1] of n equal steps, h = (t1 - t0) / n, f_i = f(t_i, y_i):
  steps 0 .. min(n, 3) - 1   a 3/8-rule rk4 step (fixed_methods_ref.TABLEAUS["rk4"]) whose k_1 = f_i is kept;
  steps i >= 3               y_{i+1} = y_i + h (55 f_i - 59 f_{i-1} + 37 f_{i-2} - 9 f_{i-3}) / 24, one evaluation.
The history restarts at every interval of t.  The adjoint is the augmented system (y, a, dL/dtheta) integrated backwards
with the same method on the same grid - what odeint_adjoint discretises - so its float64 run is the ground truth of the
adjoint gradients, and autograd through `odeint` the ground truth of the backprop gradients.  Nothing here knows the product:
the coefficients are written out again."""
import torch

import fixed_methods_ref as R

BETA = (55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0)      # weights of f_i, f_{i-1}, f_{i-2}, f_{i-3}
START = 3                                                         # rk4 steps before the first multistep step
METHOD = "explicit_adams"


def nfe(n):
    """Evaluations of an n-step solve of one interval."""
    return 4 * min(n, START) + max(n - START, 0)


def record_floats(n, step, nd):
    """Offset in floats of step `step`'s record in the compact record of an n-step solve (step = n: the total): a start-up
    step keeps [y | k_1..k_4] (5 nd), a multistep step [y | f] (2 nd)."""
    return (5 * min(step, START) + 2 * max(step - START, 0)) * nd


def solve(func, y, t0, t1, n):
    """n steps from t0 to t1; a state is a tensor or a tuple of tensors."""
    c, a, b = R.TABLEAUS["rk4"]
    like = R._tup(y)[0]
    h = (t1 - t0) / n
    fs = []                                                       # f_{i-1}, f_{i-2}, f_{i-3}
    for i in range(n):
        t = t0 + i * h
        if i < START:
            ks = []
            for s in range(4):
                ys = R._axpy(y, [(h * a[s][j], ks[j]) for j in range(s) if a[s][j] != 0.0])
                ks.append(func(torch.tensor(t + c[s] * h, dtype=like.dtype), ys))
            y = R._axpy(y, [(h * b[s], ks[s]) for s in range(4)])
            fs.insert(0, ks[0])
        else:
            fs.insert(0, func(torch.tensor(t, dtype=like.dtype), y))
            y = R._axpy(y, [(h * BETA[j], fs[j]) for j in range(4)])
            fs.pop()
    return y


def odeint(func, y0, t, step_size=None):
    """The stack of y(t_i); differentiable by torch autograd (the ground truth of backprop through the solve)."""
    outs = [y0]
    for i in range(1, len(t)):
        outs.append(solve(func, outs[-1], t[i - 1], t[i], R.grid_steps(t[i - 1], t[i], step_size)))
    return torch.stack(outs)


def adjoint_grads(func, params, ys, t, gbar, step_size=None):
    """fixed_methods_ref.adjoint_grads under this method: -> (dL/dy0, [dL/dparam])."""
    params = tuple(params)

    def aug(tt, state):
        y, a = state[0], state[1]
        with torch.enable_grad():
            y_ = y.detach().requires_grad_(True)
            f = func(tt, y_)
            vj = torch.autograd.grad(f, (y_,) + params, -a, allow_unused=True)
        vj = [torch.zeros_like(x) if v is None else v for v, x in zip(vj, (y_,) + params)]
        return (f.detach(),) + tuple(vj)

    ys, gbar = ys.detach(), gbar.detach()
    state = (ys[-1], gbar[-1].clone()) + tuple(torch.zeros_like(p) for p in params)
    for i in range(len(t) - 1, 0, -1):
        state = (ys[i],) + tuple(state[1:])
        state = solve(aug, state, t[i], t[i - 1], R.grid_steps(t[i], t[i - 1], step_size))
        state = (state[0], state[1] + gbar[i - 1]) + tuple(state[2:])
    return state[1], list(state[2:])


def reference_runs(make_ref, x0, t, Rw, step_size, adjoint, params_of=None):
    """fixed_methods_ref.reference_runs under this method: [(outputs, dL/dx0, [dL/dparam]) in float32, the same in float64]."""
    res = []
    for dtype in (torch.float32, torch.float64):
        ref = make_ref(dtype)
        params = list(params_of(ref) if params_of is not None else ref.parameters())
        x = x0.detach().cpu().to(dtype).requires_grad_(True)
        out = odeint(ref, x, t, step_size)
        if adjoint:
            gx, gp = adjoint_grads(ref, params, out, t, Rw.to(dtype), step_size)
        else:
            g = torch.autograd.grad((out * Rw.to(dtype)).sum(), [x] + params)
            gx, gp = g[0], list(g[1:])
        res.append((out.detach(), gx.detach(), [v.detach() for v in gp]))
    return res
