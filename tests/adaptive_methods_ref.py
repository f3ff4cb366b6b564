"""The adaptive methods restated for the tests: Bogacki-Shampine 3(2), Heun-Euler 2(1) and Dormand-Prince 5(4) as plain
loops over a tableau in FSAL form, in whatever dtype the state has, for any callable func(t, y) -> dy/dt (t a 0-dim tensor).
A state is a tensor or a tuple of tensors.  Nothing here knows the product: the tableaus are written out again, the
controller is the textbook one the issue of these methods states (per-tensor RMS error ratio over atol + rtol max(|y0|, |y1|),
safety 0.9, growth at most 10, shrink at most 0.2, exponent 1/p for the step size and for the initial step; dopri5 1/5 and
1/5), the interval ends on a step that may overshoot and is interpolated (cubic Hermite through (y_n, f_n, y_{n+1}, f_{n+1});
dopri5: its quartic through the mid-point too), the adjoint is the augmented system (y, a, a_t, dL/dtheta) integrated
backwards with the same method, and autograd through `odeint` is the ground truth of backprop through the solve.

forced: an attempt sequence [(|dt|, accepted, ...), ...] taken instead of the controller's - what the product's TRACE records,
so that float32 and float64 runs discretise exactly as the product did.  Every solve returns the sequence it took."""
import math

import torch

from fixed_methods_ref import _axpy, _tup

TABLEAUS = {        # name: (c, a, b, e = b - b*, order p)
    "dopri5": ([0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0],
               [[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9],
                [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
                [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
                [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]],
               [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0],
               [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720,
                -2187 / 6784 + 12231 / 42400, 11 / 84 - 649 / 6300, -1 / 60], 5),
    "bosh3": ([0.0, 1 / 2, 3 / 4, 1.0], [[], [1 / 2], [0, 3 / 4], [2 / 9, 1 / 3, 4 / 9]], [2 / 9, 1 / 3, 4 / 9, 0],
              [2 / 9 - 7 / 24, 1 / 3 - 1 / 4, 4 / 9 - 1 / 3, -1 / 8], 3),
    "adaptive_heun": ([0.0, 1.0, 1.0], [[], [1.0], [1 / 2, 1 / 2]], [1 / 2, 1 / 2, 0], [-1 / 2, 1 / 2, 0], 2),
}
CODES = {"dopri5": 0, "bosh3": 1, "adaptive_heun": 2}        # GODE_RKA_* of include/graphode.h
STAGES = {m: len(TABLEAUS[m][0]) for m in TABLEAUS}
DP_MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
          187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]


def interp_weights(method, x):
    """(cy0, cy1, kc[S]) of the end-of-interval fit at abscissa x: cy0 y_n + cy1 y_{n+1} + h sum kc_s k_s."""
    S = STAGES[method]
    x2, x3 = x * x, x * x * x
    if method != "dopri5":                          # cubic Hermite: f_n = k_1, f_{n+1} = k_S
        kc = [0.0] * S
        kc[0], kc[S - 1] = x3 - 2 * x2 + x, x3 - x2
        return 2 * x3 - 3 * x2 + 1, -2 * x3 + 3 * x2, kc
    x4 = x2 * x2
    wm = 16 * x4 - 32 * x3 + 16 * x2               # weight of y_mid = y_n + h sum DP_MID k in the quartic
    kc = [wm * m for m in DP_MID]
    kc[0] += -2 * x4 + 5 * x3 - 4 * x2 + x
    kc[6] += 2 * x4 - 3 * x3 + x2
    return -8 * x4 + 18 * x3 - 11 * x2 + 1 + wm, -8 * x4 + 14 * x3 - 5 * x2, kc


def _groups(y, groups):
    return groups if groups is not None else [[c] for c in range(len(_tup(y)))]


def _group_rms(v, y0, y1, rtol, atol, groups):
    """RMS of v / tol per group of state tensors (a group pools its tensors' elements)."""
    v, y0 = _tup(v), _tup(y0)
    y1 = _tup(y1) if y1 is not None else [None] * len(v)
    out = []
    for grp in _groups(y0, groups):
        ss = sum(float((((v[c] / (atol + rtol * (y0[c].abs() if y1[c] is None else torch.maximum(y0[c].abs(), y1[c].abs()))))
                         ) ** 2).sum()) for c in grp)
        out.append(math.sqrt(ss / sum(v[c].numel() for c in grp)))
    return out


def initial_step(func, t0, y, f0, rtol, atol, sgn, p, groups=None):
    """Hairer-Norsett-Wanner II.4 with the norms per state tensor; the last exponent is 1/p."""
    like = _tup(y)[0]
    d0 = _group_rms(y, y, None, rtol, atol, groups)
    d1 = _group_rms(f0, y, None, rtol, atol, groups)
    if max(d0) < 1e-5 or max(d1) < 1e-5:
        h0 = 1e-6
    else:
        h0 = 0.01 * max(a / b if b != 0 else float("inf") for a, b in zip(d0, d1))
    f1 = func(torch.tensor(t0 + sgn * h0, dtype=like.dtype), _axpy(y, [(sgn * h0, f0)]))
    diff = tuple(a - b for a, b in zip(_tup(f1), _tup(f0)))
    d2 = [v / h0 for v in _group_rms(diff if isinstance(y, tuple) else diff[0], y, None, rtol, atol, groups)]
    if max(d1) <= 1e-15 and max(d2) <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1 + d2)) ** (1.0 / p)
    return min(100 * h0, h1)


def optimal_step(last, ratio, p, safety=0.9, ifactor=10.0, dfactor=0.2):
    """ratio: the largest mean squared error ratio of the attempt."""
    if ratio == 0:
        return last * ifactor
    if ratio < 1:
        dfactor = 1.0
    return last / max(1.0 / ifactor, min(math.sqrt(ratio) ** (1.0 / p) / safety, 1.0 / dfactor))


def solve(func, y, t0, t1, method, rtol, atol, forced=None, groups=None, probe=True):
    """One interval -> (y(t1), attempts [(|dt|, accepted, ratio)], nfe).  probe=False skips the initial-step evaluation (a
    forced run does not need its value; nfe then does not count it)."""
    c, a, b, e, p = TABLEAUS[method]
    S = len(c)
    like = _tup(y)[0]
    tt = lambda v: torch.tensor(v, dtype=like.dtype)      # noqa: E731
    sgn = 1.0 if t1 >= t0 else -1.0
    span = abs(t1 - t0)
    k1 = func(tt(t0), y)
    nfe = 1
    if forced is not None and not probe:
        dt = float(forced[0][0])
    else:
        dt = initial_step(func, t0, y, k1, rtol, atol, sgn, p, groups)
        nfe += 1
        if forced is not None:
            dt = float(forced[0][0])
    tau, seq = 0.0, []
    while tau < span:
        h, t = sgn * dt, t0 + sgn * tau
        ks = [k1]
        for s in range(1, S):
            ks.append(func(tt(t + c[s] * h), _axpy(y, [(h * a[s][j], ks[j]) for j in range(s) if a[s][j] != 0.0])))
        nfe += S - 1
        y1 = _axpy(y, [(h * b[s], ks[s]) for s in range(S) if b[s] != 0.0])
        zero = tuple(torch.zeros_like(v) for v in _tup(y))
        err = _axpy(zero if isinstance(y, tuple) else zero[0], [(h * e[s], ks[s]) for s in range(S) if e[s] != 0.0])
        with torch.no_grad():
            ratios = [r * r for r in _group_rms(err, y, y1, rtol, atol, groups)]
        ratio = max(ratios)
        accept = all(r <= 1.0 for r in ratios) if forced is None else bool(forced[len(seq)][1])
        seq.append((dt, accept, ratio))
        if accept:
            if tau + dt >= span:
                x = (span - tau) / dt
                if x < 1.0:
                    cy0, cy1, kc = interp_weights(method, x)
                    ys = [cy0 * u + cy1 * v for u, v in zip(_tup(y), _tup(y1))]
                    for s in range(S):
                        if kc[s] != 0.0:
                            ys = [o + (h * kc[s]) * kk for o, kk in zip(ys, _tup(ks[s]))]
                    y1 = tuple(ys) if isinstance(y, tuple) else ys[0]
                return y1, seq, nfe
            y, k1 = y1, ks[S - 1]
            tau += dt
        dt = optimal_step(dt, ratio, p) if forced is None else float(forced[min(len(seq), len(forced) - 1)][0])
    return y, seq, nfe


def odeint(func, y0, t, method, rtol, atol, forced=None, probe=True):
    """(stack of y(t_i), [attempts per interval], nfe); differentiable by torch autograd (the step sizes are Python floats:
    constants of the derivative) - the ground truth of backprop through the solve.  forced: one sequence per interval."""
    outs, seqs, nfe = [y0], [], 0
    for i in range(1, len(t)):
        y, seq, n = solve(func, outs[-1], t[i - 1], t[i], method, rtol, atol, None if forced is None else forced[i - 1],
                          probe=probe)
        outs.append(y)
        seqs.append(seq)
        nfe += n
    return torch.stack(outs), seqs, nfe


def adjoint_grads(func, params, ys, t, gbar, method, rtol, atol, forced=None, probe=True):
    """What odeint_adjoint computes: the augmented state (y, a, a_t, dL/dparams) integrated backwards over every interval
    with the same method, y reset to the stored output and a incremented by its cotangent at every output time; error
    groups y, a, a_t and the parameters pooled.  forced: one sequence per interval IN THE ORDER SOLVED (last interval
    first).  -> (dL/dy0, [dL/dparam], [attempts per interval in that order])."""
    params = tuple(params)

    def aug(tt, state):
        y, a = state[0], state[1]
        with torch.enable_grad():
            y_ = y.detach().requires_grad_(True)
            t_ = tt.detach().clone().requires_grad_(True)
            f = func(t_, y_)
            vj = torch.autograd.grad(f, (t_, y_) + params, -a, allow_unused=True)
        vj = [torch.zeros_like(x) if v is None else v for v, x in zip(vj, (t_, y_) + params)]
        return (f.detach(), vj[1], vj[0].reshape(1)) + tuple(vj[2:])

    ys, gbar = ys.detach(), gbar.detach()
    groups = [[0], [1], [2]] + ([list(range(3, 3 + len(params)))] if params else [])
    state = (ys[-1], gbar[-1].clone(), torch.zeros(1, dtype=ys.dtype)) + tuple(torch.zeros_like(p) for p in params)
    seqs = []
    for n, i in enumerate(range(len(t) - 1, 0, -1)):
        with torch.no_grad():
            f_end = func(torch.tensor(t[i], dtype=ys.dtype), ys[i])
        state = (ys[i], state[1], state[2] - (f_end * gbar[i]).sum().reshape(1)) + tuple(state[3:])
        state, seq, _ = solve(aug, state, t[i], t[i - 1], method, rtol, atol, None if forced is None else forced[n], groups,
                              probe=probe)
        seqs.append(seq)
        state = (state[0], state[1] + gbar[i - 1]) + tuple(state[2:])
    return state[1], list(state[3:]), seqs


def reference_runs(make_ref, x0, t, R, method, rtol, atol, adjoint, forced_f, forced_b=None, params_of=None):
    """[(outputs, dL/dx0, [dL/dparam]) in float32, the same in float64] of the restatement make_ref(dtype) on the forced
    attempt sequences (forward: forced_f, one per interval; the adjoint solves: forced_b, in the order solved), L = sum_i
    <y(t_i), R_i>; adjoint: the gradients odeint_adjoint's discretisation gives, else autograd through odeint."""
    res = []
    for dtype in (torch.float32, torch.float64):
        ref = make_ref(dtype)
        params = list(params_of(ref) if params_of is not None else ref.parameters())
        x = x0.detach().cpu().to(dtype).requires_grad_(True)
        out, _, _ = odeint(ref, x, t, method, rtol, atol, forced_f, probe=False)
        if adjoint:
            gx, gp, _ = adjoint_grads(ref, params, out, t, R.to(dtype), method, rtol, atol, forced_b, probe=False)
        else:
            g = torch.autograd.grad((out * R.to(dtype)).sum(), [x] + params)
            gx, gp = g[0], list(g[1:])
        res.append((out.detach(), gx.detach(), [v.detach() for v in gp]))
    return res
