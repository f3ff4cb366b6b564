"""Fused backprop through rk4 and dopri5 solves of the GAT ODE function, one head and H heads, on launch-bound graphs
(gat_ode.GatOdeField; csrc/gat_driver.hip, csrc/gat_small.hip: gode_gat_small_close_stages_f32) on the GPU, against
autograd through oracle.layers_ref.gat_odefunc / gat_multihead_odefunc and oracle.solver_ref on the CPU in float32 and
float64 (unchanged).

Bar: noise_floor_check of tests/test_gpu_gcn.py with its default slack 4 - the error against float64 within 4 x the float32
oracle's own error + 1e-5 x scale.

Graphs: T1 - 37 nodes, 600 edges, one target with 300 incoming edges, a node without incoming and one without outgoing
edges, duplicate edges; T2 - tests/golden/gat_heads.npz (50 nodes); T3 - 300 nodes, 9 000 random edges (with H heads the
raw-logit route).  Widths (d, H): (16, 1), (64, 1), (32, 4), (64, 8)."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_gcn import noise_floor_check
from test_gpu_large_adjoint import profiled

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WIDTHS = [(16, 1), (64, 1), (32, 4), (64, 8)]
CLOSE = 11                                           # GODE_PROF_GAT_STEP_CLOSE
MEMBERS = ("rk4_forward_save", "rk4_backprop", "dopri5_step_backprop", "dopri5_backprop_work", "packed_grads",
           "packed_param_grads")


def close(a, b, tol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item()
    assert err <= tol * max(1.0, b.abs().max().item()), "%s: max abs err %.3e" % (what, err)


def check(got, ref32, ref64, what):
    """noise_floor_check, the figures printed first."""
    e_ref = (ref32.double() - ref64).abs().max().item()
    e_got = (got.detach().cpu().double() - ref64).abs().max().item()
    print("%-36s err %.3e  float32 oracle err %.3e  scale %.2e" % (what, e_got, e_ref, max(1.0, ref64.abs().max().item())))
    noise_floor_check(got, ref32, ref64, what)


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def _mtgt(n, tgt, dtype=torch.float32):
    E = tgt.numel()
    return torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(E)]), torch.ones(E, dtype=dtype), (n, E))


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n, src, tgt) on the CPU, int64."""
    if name == "T1":
        n, E = 37, 600
        g = torch.Generator().manual_seed(21)
        src = torch.randint(0, n - 1, (E,), generator=g)               # node 36 has no outgoing edge
        tgt = torch.randint(1, n, (E,), generator=g)                   # node 0 has no incoming edge
        hub = torch.randperm(E, generator=g)[:300]
        tgt[hub] = 5
        src[-40:], tgt[-40:] = src[:40], tgt[:40]                      # duplicate edges
        assert (tgt == 5).sum() >= 300 and not (tgt == 0).any() and not (src == n - 1).any()
        assert torch.unique(torch.stack([src, tgt]), dim=1).shape[1] < E
        return n, src, tgt
    if name == "T2":
        import os
        g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gat_heads.npz")))
        return int(g["n"]), torch.from_numpy(g["src"]).long(), torch.from_numpy(g["tgt"]).long()
    n, E = 300, 9000
    g = torch.Generator().manual_seed(22)
    return n, torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)


def names(f):
    """Parameter names in func.parameters() order (the order odeint and packed_param_grads return gradients in)."""
    return [k for k, _ in f.named_parameters()]


def product(gname, d, H, seed=5, module="auto"):
    """The product's ODE function on the GPU with its graph set (gat_models.ODEfunc for one head, gat_heads.ODEfunc for H)."""
    from graph_odenet_amd import gat_heads, gat_models
    n, src, tgt = graph(gname)
    torch.manual_seed(seed)
    f = gat_models.ODEfunc(d) if (H == 1 and module != "heads") else gat_heads.ODEfunc(d, H)
    with torch.no_grad():                                              # GroupNorm's affine pair away from (1, 0)
        f.norm1.weight.add_(0.3 * torch.randn(d))
        f.norm1.bias.add_(0.3 * torch.randn(d))
    f = f.to(DEV)
    f.set_adj(src.to(DEV), tgt.to(DEV), _mtgt(n, tgt).to(DEV))
    return f


class Ref(torch.nn.Module):
    """The oracle's function of the same parameters on the CPU in `dtype`."""

    def __init__(self, f, gname, dtype):
        super().__init__()
        self.keys = names(f)
        self.p = torch.nn.ParameterList([torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in f.parameters()])
        n, self.src, self.tgt = graph(gname)
        self.Mtgt, self.dtype = _mtgt(n, self.tgt, dtype), dtype
        self.H = len(f.gc1.heads) if hasattr(f.gc1, "heads") else 0       # 0: the reference's own one-head layer

    def forward(self, t, x):
        from oracle import layers_ref as R
        p = dict(zip(self.keys, self.p))
        gn = (p["norm1.weight"], p["norm1.bias"])
        four = ("f.weight", "f.bias", "w.weight", "w.bias")
        if self.H == 0:
            return R.gat_odefunc(t, x, self.src, self.tgt, self.Mtgt, *gn, *[p["gc1." + k] for k in four])
        heads = [[p["gc1.heads.%d.%s" % (h, k)] for k in four] for h in range(self.H)]
        return R.gat_multihead_odefunc(t, x, self.src, self.tgt, self.Mtgt, *gn, heads)

    def grads(self):
        return {k: p.grad.clone() for k, p in zip(self.keys, self.p)}


def refs(f, gname):
    return [Ref(f, gname, dt) for dt in (torch.float32, torch.float64)]


def x0_of(gname, d, seed=9, scale=0.5):
    """A start state.  At d = 64 GroupNorm(32, 64) has two channels per group and its backward scales with 1 / |x_a - x_b|
    of a pair: on plain random states some of the 300 x 32 pairs nearly coincide and the float32 oracle's own x-gradient of
    an rk4 solve sits 78 (of 2.9e3) from float64, a bar that shows nothing.  So the two channels of every pair start 6 apart
    (+-3 around the random state, the sign drawn per node and pair, so that the normalised rows - and with them the logits -
    still differ from node to node); f is a weighted mean of relu's, of order 1 over the unit interval, and no pair meets."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(graph(gname)[0], d, generator=g) * scale
    if d == 64:
        s = 3.0 * (2.0 * torch.randint(0, 2, (x.shape[0], d // 2), generator=g) - 1.0)
        x[:, 0::2] += s
        x[:, 1::2] -= s
    return x


def param_grads(f):
    return {k: p.grad.clone() for k, p in f.named_parameters()}


# ---- 2. the closing kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 4, 7])
@pytest.mark.parametrize("n,d,H", [(37, 16, 1), (163, 64, 8), (4500, 16, 2)])
def test_close_stages_against_the_one_slot_kernel(n, d, H, q):
    """theta += sum_s k_theta(slot s, ts[s]) against the float64 sum of the one-slot kernel's results (no knowledge of the
    partial layout); for q <= 4 bit for bit the four-slot closing launch with unit weights."""
    from graph_odenet_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 * n + d + q)
    groups, eps = min(32, d), 1e-5
    f = dict(dtype=torch.float32, device=DEV)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)      # noqa: E731
    gamma, beta = 1 + 0.3 * rnd(d), 0.3 * rnd(d)
    Wsrc, Wtgt, Wlog = rnd(d + 1, d) / d ** 0.5, rnd(d + 1, d) / d ** 0.5, rnd(d + 1, 2 * H) / d ** 0.5
    slot = lib.gode_gat_small_parts(n, d) * lib.gode_gat_small_part_len(d, H)
    if (n, d) == (4500, 16):
        assert lib.gode_gat_small_parts(n, d) == 512                   # the cap: a wave of the VJP launch owns several rows
    parts = torch.full((q * slot,), float("nan"), **f)
    ka = torch.empty(n, d, **f)
    for s in range(q):
        ops.gat_dense_vjp_small([(1.0, rnd(n, d))], n, d, groups, eps, gamma, beta, Wsrc, Wtgt, Wlog, H, rnd(n, d), rnd(n, d),
                                rnd(n, 2 * H), ka, parts[s * slot:(s + 1) * slot])
    ts = [0.1 + 0.17 * s for s in range(q)]
    nth = lib.gode_gat_ode_theta_len_heads(d, H)
    theta0 = torch.randn(nth + 7, generator=g)                         # non-zero, and a tail the launch must leave alone
    ref32, ref64 = theta0[:nth].clone(), theta0[:nth].double()
    kth, kat = torch.empty(nth, **f), torch.empty(1, **f)
    for s in range(q):
        ops.gat_small_finish(parts[s * slot:(s + 1) * slot], n, d, H, ts[s], kth, kat)
        ref32 += kth.cpu()
        ref64 += kth.cpu().double()
    outs = []
    for _ in range(2):
        th = theta0.to(DEV).clone()
        ops.gat_small_close_stages(parts, n, d, H, ts, th)
        outs.append(th)
    assert torch.equal(outs[0], outs[1]), "not deterministic"
    assert torch.equal(outs[0][nth:].cpu(), theta0[nth:]), "the tail after theta was touched"
    assert bool(torch.isfinite(outs[0]).all())
    check(outs[0][:nth], ref32, ref64, "close %d slots n=%d d=%d H=%d" % (q, n, d, H))
    if q <= 4:
        th, at = theta0[:nth].to(DEV).clone(), torch.zeros(1, **f)
        ops.gat_small_finish_step(parts, n, d, H, ts, [1.0] * q, th, at)
        assert torch.equal(th, outs[0][:nth]), "differs from the four-slot closing launch with unit weights"


# ---- 3. the reverse of one stage -------------------------------------------------------------------------------------------
def step_backprop(fwd, y, k, g, wk, first, t, h, wy=0.0):
    """One call of the field's dopri5_step_backprop -> (ybar_n, kbar_1 or None, theta), cloned."""
    theta = fwd.packed_grads(DEV)
    work = fwd.dopri5_backprop_work(y)
    ybar_n, kbar1 = fwd.dopri5_step_backprop(y, k, g, None, wy, wk, t, h, first, work, 0, theta)
    return ybar_n.clone(), (None if kbar1 is None else kbar1.clone()), theta.clone()


@pytest.mark.parametrize("d,H", WIDTHS)
@pytest.mark.parametrize("gname", ["T1", "T3"])
def test_stage_reverse_against_autograd(gname, d, H):
    """first = 1, wk = [1, 0, ..], no kbar7, wy = 0: J^T g and (df/dtheta)^T g of one evaluation."""
    f = product(gname, d, H)
    n = graph(gname)[0]
    x0 = x0_of(gname, d)
    g0 = torch.randn(n, d, generator=torch.Generator().manual_seed(4))
    t = 0.375
    fwd = f.gode_fields(x0.to(DEV))[0]
    assert fwd.dopri5_step_backprop is not None and fwd.small()
    assert fwd.raw_logits() == (gname == "T3" and H > 1)
    fwd.prepare()
    y, g = x0.to(DEV), g0.to(DEV)
    k = [torch.zeros_like(y) for _ in range(7)]
    runs = [step_backprop(fwd, y, k, g, [1.0] + [0.0] * 6, True, t, 0.25) for _ in range(2)]
    assert runs[0][1] is None
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2]), "not deterministic"
    got = dict(zip(names(f), fwd.packed_param_grads(runs[0][2])), x=runs[0][0])
    want = []
    for ref in refs(f, gname):
        x = x0.detach().clone().to(ref.dtype).requires_grad_(True)
        (ref(torch.tensor(t, dtype=ref.dtype), x) * g0.to(ref.dtype)).sum().backward()
        want.append(dict(ref.grads(), x=x.grad))
    for key in got:
        check(got[key], want[0][key], want[1][key], "stage %s d=%d H=%d %s" % (gname, d, H, key))


@pytest.mark.parametrize("gname,d,H", [("T1", 32, 4), ("T3", 64, 1), ("T3", 64, 8)])
def test_stage_chain_with_a_three_term_input(gname, d, H):
    """wk = [0, 0, 1, 0, ..], not first: stage 3 (input y + h (3/40 k_1 + 9/40 k_2): three terms) is swept, then stage 2 through
    the k_2 it read; k_1 is a given array whose cotangent leaves as kbar_1.  The oracle differentiates
    <f(t_3, y + h (a31 k1 + a32 f(t_2, y + h a21 k1))), g> with respect to y, k1 and the parameters."""
    from graph_odenet_amd.solver import DP_A, DP_C
    f = product(gname, d, H)
    n = graph(gname)[0]
    x0, k1 = x0_of(gname, d), x0_of(gname, d, seed=10)
    g0 = torch.randn(n, d, generator=torch.Generator().manual_seed(4))
    t, h = 0.25, 0.5
    fwd = f.gode_fields(x0.to(DEV))[0]
    fwd.prepare()
    y, g = x0.to(DEV), g0.to(DEV)
    k = [torch.zeros_like(y) for _ in range(7)]
    k[0].copy_(k1)
    fwd.eval(t + DP_C[1] * h, [[(1.0, y), (h * DP_A[1][0], k[0])]], [k[1]])
    ybar_n, kbar1, theta = step_backprop(fwd, y, k, g, [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], False, t, h)
    got = dict(zip(names(f), fwd.packed_param_grads(theta)), x=ybar_n, k1=kbar1)
    want = []
    for ref in refs(f, gname):
        dt = ref.dtype
        x, kk = x0.detach().clone().to(dt).requires_grad_(True), k1.detach().clone().to(dt).requires_grad_(True)
        k2 = ref(torch.tensor(t + DP_C[1] * h, dtype=dt), x + h * DP_A[1][0] * kk)
        k3 = ref(torch.tensor(t + DP_C[2] * h, dtype=dt), x + h * (DP_A[2][0] * kk + DP_A[2][1] * k2))
        (k3 * g0.to(dt)).sum().backward()
        want.append(dict(ref.grads(), x=x.grad, k1=kk.grad))
    for key in got:
        check(got[key], want[0][key], want[1][key], "chain %s d=%d H=%d %s" % (gname, d, H, key))


# ---- whole solves ------------------------------------------------------------------------------------------------------------
def solve_run(f, x0, R, t, method=None, step_size=None, tol=1e-5, replay=None):
    """odeint with gradients -> (gradients and outputs, (nfe forward, nfe backward), launch kinds, attempt sequences)."""
    from graph_odenet_amd import odeint as OI, solver
    f.zero_grad(set_to_none=True)
    x = x0.to(DEV).requires_grad_(True)
    f.nfe = 0
    solver.TRACE = []
    solver.REPLAY = [list(seq) for seq in replay] if replay is not None else None
    try:
        with profiled() as kinds:
            out = OI.odeint(f, x, torch.tensor(t, device=DEV), rtol=tol, atol=tol, method=method,
                            options=None if step_size is None else {"step_size": step_size})
            nfe_f = f.nfe
            assert out.grad_fn is not None
            (out * R.to(DEV)).sum().backward()
        trace = solver.TRACE
    finally:
        solver.TRACE = solver.REPLAY = None
    g = param_grads(f)
    g.update(x=x.grad.clone(), y=out.detach().clone())
    return g, (nfe_f, f.nfe - nfe_f), [k & 0xff for k in kinds], trace


def plain_solve(f, x0, t, method=None, step_size=None, tol=1e-5):
    from graph_odenet_amd import odeint as OI
    with torch.no_grad():
        out = OI.odeint(f, x0.to(DEV), torch.tensor(t, device=DEV), rtol=tol, atol=tol, method=method,
                        options=None if step_size is None else {"step_size": step_size})
    assert out.grad_fn is None
    return out


def unrolled_rk4(ref, x0, R, t, step):
    """Autograd through the oracle's 3/8-rule steps on the grid odeint takes, loss sum_i <y(t_i), R_i>."""
    from oracle import solver_ref as S
    dt = ref.dtype
    ref.zero_grad(set_to_none=True)
    x = x0.detach().clone().to(dt).requires_grad_(True)
    y, outs = x, [x]
    for i in range(1, len(t)):
        n = int(round((t[i] - t[i - 1]) / step))
        hh = (t[i] - t[i - 1]) / n
        for j in range(n):
            y = y + S.rk4_38_step(lambda tt, yy: (ref(tt, yy[0]),), torch.tensor(t[i - 1] + j * hh, dtype=dt),
                                  torch.tensor(hh, dtype=dt), (y,))[0]
        outs.append(y)
    out = torch.stack(outs)
    (out * R.to(dt)).sum().backward()
    return dict(ref.grads(), x=x.grad.clone(), y=out.detach())


RK4_T = [0.0, 0.5, 1.0]


@functools.lru_cache(maxsize=None)
def rk4_case(gname, d, H):
    """t = [0, .5, 1], step 0.25, a random cotangent on every output time: the product, inputs and the two oracle runs."""
    f = product(gname, d, H)
    x0 = x0_of(gname, d)
    R = torch.randn((3,) + tuple(x0.shape), generator=torch.Generator().manual_seed(4))
    want = [unrolled_rk4(ref, x0, R, RK4_T, 0.25) for ref in refs(f, gname)]
    return f, x0, R, want


@pytest.mark.parametrize("d,H", WIDTHS)
@pytest.mark.parametrize("gname", ["T1", "T3"])
def test_rk4_against_unrolled_autograd(gname, d, H, monkeypatch):
    f, x0, R, want = rk4_case(gname, d, H)
    fwd = f.gode_fields(x0.to(DEV))[0]
    assert fwd.rk4_forward_save is not None                            # fails on a tree without the sweep
    assert fwd.raw_logits() == (gname == "T3" and H > 1)

    def boom(self, t, x):
        raise AssertionError("ODEfunc.forward was called")
    monkeypatch.setattr(type(f), "forward", boom)
    got, nfe, kinds, _ = solve_run(f, x0, R, RK4_T, "rk4", 0.25)
    assert nfe == (16, 0)
    assert kinds.count(CLOSE) == 4, "one closing launch per step"
    assert torch.equal(got["y"], plain_solve(f, x0, RK4_T, "rk4", 0.25)), "forward differs from odeint under no_grad"
    for k in got:
        check(got[k], want[0][k], want[1][k], "rk4 %s d=%d H=%d %s" % (gname, d, H, k))


# ---- 5. dopri5 ------------------------------------------------------------------------------------------------------------------
def oracle_dopri5(ref, x0, R, tol, trace):
    from oracle import solver_ref as S
    dt = ref.dtype
    ref.zero_grad(set_to_none=True)
    x = x0.detach().clone().to(dt).requires_grad_(True)
    S.REPLAY = [list(seq) for seq in trace]
    try:
        out = S.odeint(ref, x, torch.tensor([0.0, 1.0], dtype=dt), rtol=tol, atol=tol, method="dopri5")
        assert S.REPLAY == []
    finally:
        S.REPLAY = None
    (out * R.to(dt)).sum().backward()
    return dict(ref.grads(), x=x.grad.clone(), y=out.detach().clone())


@functools.lru_cache(maxsize=None)
def dopri5_case(d, H, tol):
    """T2 under dopri5 at rtol = atol = tol: the fused run, and autograd through the oracle solver on the product's own
    attempt sequence in float32 and float64."""
    f = product("T2", d, H)
    x0 = x0_of("T2", d)
    R = torch.zeros((2,) + tuple(x0.shape))
    R[1] = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4))
    run = solve_run(f, x0, R, [0.0, 1.0], tol=tol)
    (seq,) = run[3]
    if tol == 1e-5 and (d, H) == (16, 1) and all(a[1] for a in seq):
        # (Every other width must reject by itself at the chosen x0: the test asserts it.)  One head at d = 16: one channel per GroupNorm group, so GroupNorm returns beta whatever the state, f depends on t
        # alone and no scale of x0 makes the controller reject (0.05 .. 8 tried: four attempts, all accepted, largest error
        # ratio 0.82).  The product is then made to attempt 2.5 x its third step first and to reject it (solver.REPLAY),
        # and goes on with its own sequence.
        forced = list(seq[:2]) + [(2.5 * seq[2][0], False, 0.0)] + list(seq[2:])
        run = solve_run(f, x0, R, [0.0, 1.0], tol=tol, replay=[forced])
    want = [oracle_dopri5(ref, x0, R, tol, run[3]) for ref in refs(f, "T2")]
    return f, x0, R, run, want


@pytest.mark.parametrize("tol", [1e-3, 1e-5])
@pytest.mark.parametrize("d,H", [(32, 4), (16, 1)])
def test_dopri5_against_the_oracle_on_the_products_own_steps(d, H, tol):
    f, x0, R, (got, nfe, kinds, trace), want = dopri5_case(d, H, tol)
    (seq,) = trace
    acc = [a[0] for a in seq if a[1]]
    print("attempts %d, accepted %d, last abscissa %.3f" % (len(seq), len(acc), (1.0 - sum(acc[:-1])) / acc[-1]))
    assert len(acc) >= 2
    assert (1.0 - sum(acc[:-1])) / acc[-1] < 1.0, "the last step must overshoot t = 1 and be interpolated"
    if tol == 1e-5:
        assert sum(1 for a in seq if not a[1]) >= 1, seq
    assert kinds.count(CLOSE) == len(acc), "one closing launch per accepted step"
    assert nfe == (2 + 6 * len(seq), 0)
    assert torch.equal(got["y"], plain_solve(f, x0, [0.0, 1.0], tol=tol)), "forward differs from odeint under no_grad"
    for k in got:
        check(got[k], want[0][k], want[1][k], "dopri5 %g d=%d H=%d %s" % (tol, d, H, k))


# ---- 6. re-run mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["rk4", "dopri5"])
def test_rerun_mode_bit_identical(method, monkeypatch):
    from graph_odenet_amd import odeint as OI
    if method == "rk4":
        f, x0, R, _ = rk4_case("T3", 32, 4)
        args = (RK4_T, "rk4", 0.25)
    else:
        f, x0, R, _, _ = dopri5_case(32, 4, 1e-3)
        args = ([0.0, 1.0], None, None, 1e-3)
    got, _, kinds, _ = solve_run(f, x0, R, *args)
    monkeypatch.setattr(OI, "BACKPROP_SAVE_MAX_BYTES", 0)
    rec, _, kinds_r, _ = solve_run(f, x0, R, *args)
    assert kinds_r.count(CLOSE) == kinds.count(CLOSE) > 0
    for k in got:
        assert torch.equal(rec[k], got[k]), k


# ---- 7. the same discrete gradient as the generic path -----------------------------------------------------------------------
def block_grads(blk, x0, gout, graph_args):
    blk.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    out = blk(x, *graph_args)
    out.backward(gout)
    return out.detach().clone(), x.grad.clone(), [p.grad.clone() for p in blk.parameters()]


@pytest.mark.parametrize("method,kw", [("rk4", dict(step_size=0.25)), ("dopri5", dict(tol=1e-3))])
@pytest.mark.parametrize("module,d,H", [("models", 16, 1), ("heads", 32, 4)])
def test_block_matches_the_generic_path(module, d, H, method, kw):
    """ODEBlock(adjoint=False) on T3 from gat_models and from gat_heads: the fused sweep against the generic path (each
    interval re-run as torch ops under autograd), within the 1e-4 of test_fused_fields_agree_with_autograd_through_the_layer.
    The functions come from product(), whose GroupNorm affine pair is random.  With the default pair (1, 0) the float32
    oracle's own dbeta of this solve sits 6.9e-2 (of 17) from float64 (the fused sweep 1.6e-2, the generic path 1.3e-2:
    measured at d = 32, H = 4), so no two float32 paths can be held to 1e-4 of each other there; with a random pair the
    oracle's error is 1.4e-4 of 27 (test_rk4_against_unrolled_autograd on the same graph and width)."""
    from graph_odenet_amd import gat_ode
    from graph_odenet_amd.models import ODEBlock
    n, src, tgt = graph("T3")
    args = (src.to(DEV), tgt.to(DEV), _mtgt(n, tgt).to(DEV))
    blk = ODEBlock(product("T3", d, H, seed=8, module=module), method=method, adjoint=False, **kw).to(DEV)
    assert type(blk.odefunc).__module__.endswith("gat_" + module)
    x0 = x0_of("T3", d).to(DEV)
    gout = torch.randn(n, d, generator=torch.Generator().manual_seed(6)).to(DEV)
    with profiled() as kinds:
        fused = block_grads(blk, x0, gout, args)
    assert [k & 0xff for k in kinds].count(CLOSE) >= 1
    gat_ode.GatOdeField.BACKPROP_FUSED = False
    try:
        assert blk.odefunc.gode_fields(x0)[0].rk4_forward_save is None
        generic = block_grads(blk, x0, gout, args)
    finally:
        gat_ode.GatOdeField.BACKPROP_FUSED = True
    assert torch.equal(fused[0], generic[0]), "forward"
    close(fused[1], generic[1], 1e-4, "x")
    for (nm, _), a, b in zip(blk.named_parameters(), fused[2], generic[2]):
        close(a, b, 1e-4, nm)


# ---- 8. outside the route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["padded", "d128", "option"])
def test_outside_the_route_the_generic_path_is_unchanged(case):
    from graph_odenet_amd import _lib, gat_heads, gat_models, gat_ode
    from graph_odenet_amd.models import ODEBlock
    lib = _lib.load()
    if case == "padded":
        n, E, d, H = 5000, 24000, 32, 8
        g = torch.Generator().manual_seed(12)
        src, tgt = torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)
    else:
        n, src, tgt = graph("T1")
        d, H = (128, 1) if case == "d128" else (32, 4)
    args = (src.to(DEV), tgt.to(DEV), _mtgt(n, tgt).to(DEV))
    torch.manual_seed(8)
    blk = ODEBlock(gat_models.ODEfunc(d) if H == 1 else gat_heads.ODEfunc(d, H), method="rk4", step_size=0.5, adjoint=False).to(DEV)
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(9)).to(DEV) * 0.5
    gout = torch.randn(n, d, generator=torch.Generator().manual_seed(6)).to(DEV)
    if case == "option":
        lib.gode_set_option(b"small_fused", 0)
    try:
        blk.odefunc.set_adj(*args)
        fwd = blk.odefunc.gode_fields(x0)[0]
        assert fwd.s.pad_logits == (case == "padded")
        for name in MEMBERS:
            assert getattr(fwd, name) is None, name
        on = block_grads(blk, x0, gout, args)
        gat_ode.GatOdeField.BACKPROP_FUSED = False
        try:
            off = block_grads(blk, x0, gout, args)
        finally:
            gat_ode.GatOdeField.BACKPROP_FUSED = True
    finally:
        if case == "option":
            lib.gode_set_option(b"small_fused", 1)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    for a, b in zip(on[2], off[2]):
        assert torch.equal(a, b)


# ---- 9. the adjoint is untouched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,kw", [("rk4", dict(step_size=0.25)), ("dopri5", dict(tol=1e-4))])
@pytest.mark.parametrize("d,H", [(32, 4), (16, 1)])
def test_adjoint_native_step_matches_python_driver(d, H, method, kw):
    """ODEBlock(adjoint=True) on T2: the C drivers (whose adjoint stage is now stage_vjp + the closing part) against the
    per-stage Python drivers - same kernels in the same order, so outputs, gradients and nfe agree bit for bit."""
    from graph_odenet_amd import gat_heads, gat_models, odeint as OI, solver as PS
    from graph_odenet_amd.models import ODEBlock
    n, src, tgt = graph("T2")
    args = (src.to(DEV), tgt.to(DEV), _mtgt(n, tgt).to(DEV))
    x0 = x0_of("T2", d).to(DEV)
    gout = torch.randn(n, d, generator=torch.Generator().manual_seed(4)).to(DEV)
    res = {}
    for native in (True, False):
        PS.DOPRI5_NATIVE = OI.NATIVE_RK4 = native
        try:
            torch.manual_seed(6)
            blk = ODEBlock(gat_models.ODEfunc(d) if H == 1 else gat_heads.ODEfunc(d, H), method=method, **kw).to(DEV)
            out, gx, gp = block_grads(blk, x0, gout, args)
            res[native] = (out, gx, gp, blk.nfe)
        finally:
            PS.DOPRI5_NATIVE = OI.NATIVE_RK4 = True
    assert res[True][3] == res[False][3]
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    for a, b in zip(res[True][2], res[False][2]):
        assert torch.equal(a, b)
