"""The fixed-grid methods restated for the tests: plain loops over the stages of a Butcher tableau, in whatever dtype the
state has, for any callable func(t, y) -> dy/dt (t a 0-dim tensor).  A state is a tensor or a tuple of tensors.  Nothing
here knows the product: the tableaus are written out again, the grid rule is odeint's (step_size, or one step per
interval of t), the adjoint is the augmented system (y, a, dL/dtheta) integrated backwards with the same method, which is
what odeint_adjoint discretises - so its float64 run is the ground truth of the adjoint gradients, and autograd through
`odeint` the ground truth of the backprop gradients.

Also the helpers the GPU tests share (tests/test_gpu_fixed_methods.py): the project's noise-floor yardstick, random graphs
with self loops, and the CPU restatements of the ODE functions the fixed-grid solves are run on."""
import math

import torch

TABLEAUS = {        # name: (c, a, b)
    "rk4": ([0.0, 1 / 3, 2 / 3, 1.0], [[], [1 / 3], [-1 / 3, 1.0], [1.0, -1.0, 1.0]], [1 / 8, 3 / 8, 3 / 8, 1 / 8]),
    "euler": ([0.0], [[]], [1.0]),
    "midpoint": ([0.0, 0.5], [[], [0.5]], [0.0, 1.0]),
}
CODES = {"rk4": 0, "euler": 1, "midpoint": 2}        # GODE_RK_* of include/graphode.h
STAGES = {m: len(TABLEAUS[m][0]) for m in TABLEAUS}


def grid_steps(t0, t1, step_size):
    """Equal steps covering [t0, t1] with |h| <= step_size; one step without a step_size."""
    if step_size is None:
        return 1
    return max(int(math.ceil(abs(t1 - t0) / step_size - 1e-9)), 1)


def _tup(y):
    return y if isinstance(y, tuple) else (y,)


def _axpy(y, terms):
    """y + sum coef * k over (coef, k) pairs of states."""
    out = list(_tup(y))
    for coef, k in terms:
        out = [o + coef * kc for o, kc in zip(out, _tup(k))]
    return tuple(out) if isinstance(y, tuple) else out[0]


def solve(func, y, t0, t1, n, method):
    """n steps of `method` from t0 to t1."""
    c, a, b = TABLEAUS[method]
    like = _tup(y)[0]
    h = (t1 - t0) / n
    for i in range(n):
        t = t0 + i * h
        ks = []
        for s in range(len(c)):
            ys = _axpy(y, [(h * a[s][j], ks[j]) for j in range(s) if a[s][j] != 0.0])
            ks.append(func(torch.tensor(t + c[s] * h, dtype=like.dtype), ys))
        y = _axpy(y, [(h * b[s], ks[s]) for s in range(len(c)) if b[s] != 0.0])
    return y


def odeint(func, y0, t, method, step_size=None):
    """The stack of y(t_i); differentiable by torch autograd (the ground truth of backprop through the solve)."""
    outs = [y0]
    for i in range(1, len(t)):
        outs.append(solve(func, outs[-1], t[i - 1], t[i], grid_steps(t[i - 1], t[i], step_size), method))
    return torch.stack(outs)


def adjoint_grads(func, params, ys, t, gbar, method, step_size=None):
    """What odeint_adjoint computes: from the outputs ys (stack over t) and their cotangents gbar, the augmented state
    (y, a, dL/dparams) integrated backwards over every interval with the same method on the same grid, y reset to the
    stored output and a incremented by its cotangent at every output time.  -> (dL/dy0, [dL/dparam])."""
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
        state = solve(aug, state, t[i], t[i - 1], grid_steps(t[i], t[i - 1], step_size), method)
        state = (state[0], state[1] + gbar[i - 1]) + tuple(state[2:])
    return state[1], list(state[2:])


# ---- the yardstick (tests/test_gpu_gcn.py: noise_floor_check and close, copied) ---------------------------------------------
def noise_floor_check(got, ref32, ref64, what, slack=4.0, floor=1e-5, e_ref_draws=None):
    """|got - exact| must stay within `slack` x the fp32 restatement's own distance to the fp64 ground truth (plus 1e-5 of
    the magnitude).  The figures are printed first.  e_ref_draws: further measured samples of the fp32 restatement's error
    on the same quantity (see test_edge_block); the largest is the restatement's error."""
    got = got.detach().cpu().double()
    e_ref = (ref32.double() - ref64).abs().max().item()
    if e_ref_draws is not None:
        e_ref = max(e_ref, e_ref_draws)
    e_got = (got - ref64).abs().max().item()
    scale = max(1.0, ref64.abs().max().item())
    print("%-44s err %.3e  fp32 restatement err %.3e  scale %.2e" % (what, e_got, e_ref, scale))
    assert e_got <= slack * e_ref + floor * scale, "%s: err %.3e vs fp32-restatement err %.3e (scale %.2e)" % (what, e_got, e_ref, scale)


def close(a, b, tol=1e-5, what=""):
    a = a.detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    print("%-44s err %.3e  (bar %.1e x %.2e)" % (what, err, tol, scale))
    assert err <= tol * scale, "%s: max err %.3e (scale %.3e)" % (what, err, scale)


# ---- graphs and ODE functions ------------------------------------------------------------------------------------------------
def random_adj(n, n_edges, seed):
    """Row-normalised random adjacency with self loops, sparse COO on the CPU (duplicates coalesced)."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.cat([torch.randint(0, n, (n_edges,), generator=g), torch.arange(n)])
    cols = torch.cat([torch.randint(0, n, (n_edges,), generator=g), torch.arange(n)])
    a = torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.ones(rows.numel()), (n, n)).coalesce()
    deg = torch.zeros(n).index_add_(0, a.indices()[0], a.values())
    return torch.sparse_coo_tensor(a.indices(), a.values() / deg[a.indices()[0]], (n, n)).coalesce()


GCN_PNAMES = ("norm1.weight", "norm1.bias", "gc1.weight", "gc1.bias")


class GcnRef(torch.nn.Module):
    """oracle.layers_ref.odefunc on the parameters of a product models.ODEfunc, on the CPU in `dtype`."""

    def __init__(self, f, adj, dtype):
        super().__init__()
        sd = dict(f.named_parameters())
        self.p = torch.nn.ParameterList([torch.nn.Parameter(sd[k].detach().cpu().to(dtype).clone()) for k in GCN_PNAMES])
        self.adj, self.dtype = adj.to(dtype), dtype

    def forward(self, tt, x):
        from oracle import layers_ref as L
        return L.odefunc(tt.to(self.dtype), x, self.adj, *self.p)

    def named(self):
        return dict(zip(GCN_PNAMES, self.p))


class GcnRefBranch(GcnRef):
    """GcnRef with the branch of its relu prescribed near the kink.  relu' jumps at 0, and an fp32 evaluation of a
    pre-activation within the fp32 forward error of 0 has no determinate branch: among the 1.7e7 pre-activations of the
    large-route case some lie within 1e-7 of it.  `branches`: the [z > 0] the code under test took, one bool tensor per
    evaluation in evaluation order.  Where |z| < eps that branch is taken (either is the derivative of a computed
    solution); elsewhere the restatement's own, and `disagree` counts the elements where the two differ there - the caller
    asserts there are none.  eps = 1e-5: what the yardstick grants an fp32 forward value of magnitude 1.  The function is
    the oracle's, layer by layer (odefunc = relu(graph_convolution([t | group_norm_2d(x)])))."""

    def __init__(self, f, adj, dtype, branches, eps=1e-5):
        super().__init__(f, adj, dtype)
        self.branches, self.eps, self.disagree, self.near = list(branches), eps, 0, 0

    def forward(self, tt, x):
        from oracle import layers_ref as L
        gamma, beta, W, b = self.p
        xn = L.group_norm_2d(x, min(32, x.shape[1]), gamma, beta)
        z = L.graph_convolution(torch.cat([torch.ones_like(xn[:, :1]) * tt.to(self.dtype), xn], 1), self.adj, W, b)
        own, given = z.detach() > 0, self.branches.pop(0)
        near = z.detach().abs() < self.eps
        self.disagree += int(((own != given) & ~near).sum())
        self.near += int(((own != given) & near).sum())
        return z * torch.where(near, given, own).to(self.dtype)


class Mlp(torch.nn.Module):
    """A two-layer tanh MLP of the state and the time: a func odeint knows nothing about (the generic autograd field)."""

    def __init__(self, d, hidden=16, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.l1 = torch.nn.Linear(d + 1, hidden)
        self.l2 = torch.nn.Linear(hidden, d)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.4)

    def forward(self, t, y):
        tcol = torch.ones(y.shape[0], 1, dtype=y.dtype, device=y.device) * t.to(y.dtype)
        return self.l2(torch.tanh(self.l1(torch.cat([tcol, y], 1))))


def reference_runs(make_ref, x0, t, R, method, step_size, adjoint, params_of=None):
    """[(outputs, dL/dx0, [dL/dparam]) in float32, the same in float64] of the restatement make_ref(dtype) (an nn.Module),
    L = sum_i <y(t_i), R_i>; adjoint: the gradients odeint_adjoint's discretisation gives, else autograd through odeint.
    params_of(ref): the tensors differentiated with respect to (default: ref.parameters())."""
    res = []
    for dtype in (torch.float32, torch.float64):
        ref = make_ref(dtype)
        params = list(params_of(ref) if params_of is not None else ref.parameters())
        x = x0.detach().cpu().to(dtype).requires_grad_(True)
        out = odeint(ref, x, t, method, step_size)
        if adjoint:
            gx, gp = adjoint_grads(ref, params, out, t, R.to(dtype), method, step_size)
        else:
            g = torch.autograd.grad((out * R.to(dtype)).sum(), [x] + params)
            gx, gp = g[0], list(g[1:])
        res.append((out.detach(), gx.detach(), [v.detach() for v in gp]))
    return res


def random_edges(n, n_edges, seed):
    """(src, tgt) int64 on the CPU: random edges plus a self loop per node."""
    g = torch.Generator().manual_seed(seed)
    src = torch.cat([torch.randint(0, n, (n_edges - n,), generator=g), torch.arange(n)])
    tgt = torch.cat([torch.randint(0, n, (n_edges - n,), generator=g), torch.arange(n)])
    return src, tgt


def mtgt(n, tgt, dtype=torch.float32):
    E = tgt.numel()
    return torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(E)]), torch.ones(E, dtype=dtype), (n, E))


class GatRef(torch.nn.Module):
    """oracle.layers_ref.gat_odefunc / gat_multihead_odefunc on the parameters of a product GAT ODEfunc (one head:
    gat_models.ODEfunc, H heads: gat_heads.ODEfunc), on the CPU in `dtype`; parameters in func.parameters() order."""

    def __init__(self, f, n, src, tgt, dtype):
        super().__init__()
        self.keys = [k for k, _ in f.named_parameters()]
        self.p = torch.nn.ParameterList([torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in f.parameters()])
        self.src, self.tgt, self.Mtgt, self.dtype = src, tgt, mtgt(n, tgt, dtype), dtype
        self.H = len(f.gc1.heads) if hasattr(f.gc1, "heads") else 0

    def forward(self, t, x):
        from oracle import layers_ref as L
        p = dict(zip(self.keys, self.p))
        gn = (p["norm1.weight"], p["norm1.bias"])
        four = ("f.weight", "f.bias", "w.weight", "w.bias")
        if self.H == 0:
            return L.gat_odefunc(t, x, self.src, self.tgt, self.Mtgt, *gn, *[p["gc1." + k] for k in four])
        heads = [[p["gc1.heads.%d.%s" % (h, k)] for k in four] for h in range(self.H)]
        return L.gat_multihead_odefunc(t, x, self.src, self.tgt, self.Mtgt, *gn, heads)
