"""The adjoint ODE drivers above 65 536 rows against the oracle: odeint_adjoint (rk4 and dopri5) of the fused GCN field
on R-MAT graphs of 2^17 rows, where gode_gcn_ode_rk4_adjoint leaves the launch-bound code (two-stream schedule, the
one-pass VJP + weight-gradient branch at d = 128, the separate reductions at other widths); one stage of the augmented
field at the benchmark's 2^20 rows; the GAT ODE fields above 65 536 nodes inside an adjoint solve.  Every comparison is
against oracle/solver_ref.odeint_adjoint over oracle/layers_ref in float32 and float64 on the CPU, at the fp32
oracle's own noise floor (noise_floor_check), computed once per module."""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

PNAMES = ("norm1.weight", "norm1.bias", "gc1.weight", "gc1.bias")
T01 = [0.0, 1.0]
STEP = 0.5


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def noise_floor_check(got, ref32, ref64, what, slack=4.0, floor=1e-5):
    """|got - exact| must stay within `slack` x the fp32 oracle's own distance to the fp64 ground truth
    (plus 1e-5 of the magnitude): parity to the noise floor of the fp32 computation itself."""
    got = got.detach().cpu().double()
    e_ref = (ref32.double() - ref64).abs().max().item()
    e_got = (got - ref64).abs().max().item()
    scale = max(1.0, ref64.abs().max().item())
    print("noise floor %-40s e_got / e_ref = %.3f" % (what, e_got / max(e_ref, 1e-300)))       # margin to the bar (-s)
    assert e_got <= slack * e_ref + floor * scale, "%s: err %.3e vs fp32-oracle err %.3e (scale %.2e)" % (what, e_got, e_ref, scale)


def cpu_coo(g):
    """CPU COO copy of a CSRGraph (the oracle's adjacency)."""
    rows = torch.repeat_interleave(torch.arange(g.n_rows), (g.rowptr[1:] - g.rowptr[:-1]).cpu().long())
    return torch.sparse_coo_tensor(torch.stack([rows, g.col.cpu().long()]), g.val.cpu(), (g.n_rows, g.n_rows))


def make_func(d, adj_dev, seed=0, node_order=None):
    from graph_odenet_amd import models
    torch.manual_seed(seed)
    f = models.ODEfunc(d)
    if node_order is not None:
        f.node_order = node_order
    with torch.no_grad():
        f.norm1.weight.uniform_(0.5, 1.5)
        f.norm1.bias.uniform_(-0.5, 0.5)
    f = f.to(dev())
    f.set_adj(adj_dev)
    return f


@contextlib.contextmanager
def options(**kw):
    """gode_set_option switches for the body; the process-global values are restored however it ends."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    old = {k: lib.gode_get_option(k.encode()) for k in kw}
    try:
        for k, v in kw.items():
            assert lib.gode_set_option(k.encode(), v) == 0 and lib.gode_get_option(k.encode()) == v, k
        yield
    finally:
        for k, v in old.items():
            lib.gode_set_option(k.encode(), v)


@contextlib.contextmanager
def profiled(cap=4096):
    """Kinds (GODE_PROF_*) of the profiled launches issued in the body, in order."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    prof = lib.gode_prof_create(cap)
    assert prof
    kinds = []
    lib.gode_prof_enable(prof)
    try:
        yield kinds
        torch.cuda.synchronize()
        n = lib.gode_prof_count(prof)
        assert 0 < n < cap
        buf = (ctypes.c_int32 * n)()
        assert lib.gode_prof_kinds(prof, buf, n) == n
        kinds.extend(int(k) for k in buf)
    finally:
        lib.gode_prof_enable(None)
        lib.gode_prof_destroy(prof)


def oracle_adjoint(odefunc, args, params, x0, R, dtype, method="rk4", rtol=1e-6, atol=1e-12, opts=None):
    """y(1), dL/dx0 and dL/dparams through oracle/solver_ref.odeint_adjoint of `odefunc(t, x, *args, *params)` in
    `dtype`, L = <y(1), R>."""
    from oracle import solver_ref as S
    ps = [torch.nn.Parameter(p.detach().cpu().to(dtype).clone()) for p in params]
    args = [a.to(dtype) if torch.is_tensor(a) and a.is_floating_point() else a for a in args]

    class F(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.ParameterList(ps)

        def forward(self, tt, x):
            return odefunc(tt.to(dtype), x, *args, *self.p)
    x = x0.detach().cpu().to(dtype).clone().requires_grad_(True)
    if opts is None and method == "rk4":
        opts = {"step_size": STEP}
    out = S.odeint_adjoint(F(), x, torch.tensor(T01, dtype=dtype), rtol, atol, method, opts)[1]
    (out * R.to(dtype)).sum().backward()
    return out.detach(), x.grad, [p.grad for p in ps]


def oracle_pair(*a, **kw):
    return {dt: oracle_adjoint(*a, dtype=dt, **kw) for dt in (torch.float32, torch.float64)}


def check_vs_oracle(got, ref, names, what):
    (y, gx, gp), (o32, gx32, gp32), (o64, gx64, gp64) = got, ref[torch.float32], ref[torch.float64]
    noise_floor_check(y, o32, o64, what + " y(1)")
    noise_floor_check(gx, gx32, gx64, what + " dL/dx0")
    for k, a, b, c in zip(names, gp, gp32, gp64):
        noise_floor_check(a, b, c, what + " dL/d" + k)


def assert_equal_runs(a, b, what):
    """(y, dL/dx0, [dL/dparam], ...) of two runs bit for bit."""
    assert torch.equal(a[0], b[0]), "%s: y(1) differs" % what
    assert torch.equal(a[1], b[1]), "%s: dL/dx0 differs" % what
    for j, (p, q) in enumerate(zip(a[2], b[2])):
        assert torch.equal(p, q), "%s: dL/d%s differs" % (what, PNAMES[j])


def block_run(f, x0, R):
    """ODEBlock(f, rk4, step 0.5), adjoint on (the _last_only path of the benchmark): y(1), dL/dx0, dL/dparams, and
    nfe of the forward and of the backward pass."""
    from graph_odenet_amd import models
    blk = models.ODEBlock(f, method="rk4", step_size=STEP)
    assert blk.adjoint
    f.zero_grad(set_to_none=True)
    x = x0.detach().clone().requires_grad_(True)
    f.nfe = 0
    y = blk(x, f._gode_graph_arg)
    nfe_f = f.nfe
    f.nfe = 0
    (y * R).sum().backward()
    torch.cuda.synchronize()
    return y.detach().clone(), x.grad.clone(), [p.grad.clone() for p in f.parameters()], (nfe_f, f.nfe)


class _GcnProblem:
    def __init__(self, d, seed):
        from graph_odenet_amd import synth, odeint as OI
        g = synth.rmat_graph(17, 1 << 20, seed=1, device=dev())
        assert g.n_rows > (1 << 16)
        self.n, self.d = g.n_rows, d
        self.adj = cpu_coo(g)
        self.f = make_func(d, g, seed=seed, node_order="degree")
        self.f._gode_graph_arg = g
        assert self.f.norm1.num_groups == min(32, d)
        torch.manual_seed(seed + 100)
        self.x0 = torch.randn(g.n_rows, d, device=dev())
        self.R = torch.randn(g.n_rows, d, device=dev())
        assert OI._fields(self.f, self.x0)[0].row_order is not None, "the rows must really be renumbered"
        assert [k for k, _ in self.f.named_parameters()] == list(PNAMES)
        self.params = [p for p in self.f.parameters()]
        self._ref = None

    def ref(self):
        from oracle import layers_ref as L
        if self._ref is None:
            self._ref = oracle_pair(L.odefunc, [self.adj], self.params, self.x0, self.R.cpu())
        return self._ref


@pytest.fixture(scope="module")
def gcn128():
    p = _GcnProblem(128, seed=4)
    p.ref()
    yield p
    p._ref = None


# ---------------------------------------------------------------------------------------------------------------------
# 1. d = 128: the `bw` branch (one-pass VJP + weight gradient) and the option matrix
# ---------------------------------------------------------------------------------------------------------------------
SPMM, GEMM_FWD, GEMM_BWD, WGRAD, BWD_WGRAD = 0, 1, 2, 3, 4
SPLIT, PC = 1 << 8, 2 << 8

# Kinds each setting must and must not launch over one forward + adjoint pass (csrc/gemm.hip dispatch,
# gode_bwd_wgrad_supported: the one-pass branch needs bwd_wgrad, bwd_pc and wgrad_split == 8).  overlap and y2_colsum
# move launches between streams / change a reduction's source only: their kinds are the default's.
DEFAULT_KINDS = {SPMM, GEMM_FWD | PC, BWD_WGRAD | PC}
NON_BW = {GEMM_BWD, GEMM_BWD | PC, WGRAD, WGRAD | PC}
SETTINGS = [
    ("default", {}, DEFAULT_KINDS, NON_BW | {GEMM_FWD, GEMM_FWD | SPLIT}),
    ("overlap0", {"overlap": 0}, DEFAULT_KINDS, NON_BW),
    ("y2_colsum0", {"y2_colsum": 0}, DEFAULT_KINDS, NON_BW),
    ("bwd_wgrad0", {"bwd_wgrad": 0}, {GEMM_BWD | PC, WGRAD | PC}, {BWD_WGRAD | PC, GEMM_BWD, WGRAD}),
    ("bwd_pc0", {"bwd_pc": 0}, {GEMM_BWD, WGRAD | PC}, {BWD_WGRAD | PC, GEMM_BWD | PC}),
    ("fwd_pc0", {"fwd_pc": 0}, {GEMM_FWD | SPLIT, GEMM_FWD, BWD_WGRAD | PC}, {GEMM_FWD | PC}),
    # with the producer / consumer forward on (the default) the split-bf16 forward is never reached: gemm_split is
    # only observable with fwd_pc off
    ("gemm_split0", {"gemm_split": 0, "fwd_pc": 0}, {GEMM_FWD, BWD_WGRAD | PC}, {GEMM_FWD | PC, GEMM_FWD | SPLIT}),
    ("wgrad_split0", {"wgrad_split": 0}, {GEMM_BWD | PC, WGRAD}, {BWD_WGRAD | PC, WGRAD | PC}),
    ("wgrad_split6", {"wgrad_split": 6}, {GEMM_BWD | PC, WGRAD | PC}, {BWD_WGRAD | PC, WGRAD}),
]


@pytest.mark.parametrize("name,opts,must,must_not", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_gcn_rk4_adjoint_d128_vs_oracle(gcn128, name, opts, must, must_not):
    """R-MAT 2^17 rows, d = 128, 32 groups, hubs-first renumbering, ODEBlock rk4 step 0.5 with the adjoint, loss
    <y(1), R>: y(1), dL/dx0, dW, db, dgamma, dbeta at the oracle's noise floor under each switch setting; nfe 8 / 9;
    a profiled re-run shows the setting really changed the kernels that ran."""
    p = gcn128
    with options(**opts):
        got = block_run(p.f, p.x0, p.R)
        with profiled() as kinds:
            again = block_run(p.f, p.x0, p.R)
    assert got[3] == (8, 9), got[3]
    check_vs_oracle(got[:3], p.ref(), PNAMES, name)
    assert_equal_runs(got, again, name + ": profiled re-run")
    seen = set(kinds)
    assert must <= seen, "%s: kinds %s missing from %s" % (name, sorted(must - seen), sorted(seen))
    assert not (must_not & seen), "%s: unexpected kinds %s" % (name, sorted(must_not & seen))


def test_gcn_rk4_adjoint_d128_schedules_bit_identical(gcn128):
    """The two-stream schedule issues the launches of the one-stream schedule on the same data: every output and
    gradient bit for bit; two back-to-back default runs likewise (a race between the streams would show here);
    the bias gradient from the SpMM's column sums really is another summation than the pass over dZ."""
    p = gcn128
    with options(overlap=1):
        a = block_run(p.f, p.x0, p.R)
        b = block_run(p.f, p.x0, p.R)
    with options(overlap=0):
        c = block_run(p.f, p.x0, p.R)
    assert_equal_runs(a, b, "two default runs")
    assert_equal_runs(a, c, "overlap 1 vs 0")
    with options(y2_colsum=0):
        e = block_run(p.f, p.x0, p.R)
    assert torch.equal(a[1], e[1])
    assert not torch.equal(a[2][3], e[2][3]), "y2_colsum=0 left the bias gradient bit for bit unchanged: switch ignored?"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the non-`bw` large branch: d = 64 (32 groups) and d = 16 (16 groups)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 16])
def test_gcn_rk4_adjoint_non_bw_branch_vs_oracle(d):
    """d != 128 above 65 536 rows: Wg(g) and the next Gf on the side stream beside Gb(g), separate reductions, theta
    fix-up per stage.  overlap 1 and 0 against the oracle and bit for bit each other.  At d = 16 the state holds
    GRAPH_CAPTURE_MAX_ELEMS elements: a third call replays captured HIP graphs (overlap off inside the capture) and
    equals the first, eager two-stream call bit for bit."""
    from graph_odenet_amd import odeint as OI
    p = _GcnProblem(d, seed=20 + d)
    res = {}
    for ov in (1, 0):
        OI.plans_of(p.f).clear()
        with options(overlap=ov):
            res[ov] = block_run(p.f, p.x0, p.R)
        assert res[ov][3] == (8, 9), res[ov][3]
        assert all(pl.gf is None and pl.gb is None for pl in OI.plans_of(p.f).values())
    assert_equal_runs(res[1], res[0], "d=%d overlap 1 vs 0" % d)
    check_vs_oracle(res[1][:3], p.ref(), PNAMES, "d=%d" % d)
    if d == 16:
        assert p.n * d == OI.GRAPH_CAPTURE_MAX_ELEMS
        with options(overlap=1):
            rep = block_run(p.f, p.x0, p.R)
        plans = list(OI.plans_of(p.f).values())
        assert len(plans) == 1 and plans[0].gf is not None and plans[0].gb is not None, "solves not captured"
        assert_equal_runs(res[1], rep, "d=16 captured replay vs eager two-stream")


# ---------------------------------------------------------------------------------------------------------------------
# 3. dopri5 adjoint above 65 536 rows
# ---------------------------------------------------------------------------------------------------------------------
def test_gcn_dopri5_adjoint_large_vs_oracle():
    """d = 32, odeint_adjoint(dopri5, rtol = atol = 1e-3): gode_gcn_ode_dopri5_step_forward / _adjoint with the
    separate reductions and the multi-tensor error norm at 2^17 rows.  The product replaying the fp32 oracle's step
    sequence sits at the noise floor of the fp64 oracle replaying it too; the product's own controller walks with the
    oracle's (tests/test_gpu_gcn.py _same_steps rules).  The tolerance keeps the CPU oracle to a few accepted steps each
    way (at 1e-4 the adjoint solve takes ~70 attempts, minutes of CPU time); at least 2 are asserted, so that the
    controller stays exercised."""
    from graph_odenet_amd import odeint as OI, solver as PS
    from oracle import layers_ref as L, solver_ref as S
    tol = 1e-3
    p = _GcnProblem(32, seed=31)
    R = p.R.cpu()
    S.TRACE = []
    try:
        r32 = oracle_adjoint(L.odefunc, [p.adj], p.params, p.x0, R, torch.float32, method="dopri5", rtol=tol, atol=tol)
        ref_seq = S.TRACE
    finally:
        S.TRACE = None
    assert len(ref_seq) == 2
    for k, seq in enumerate(ref_seq):
        assert sum(1 for q in seq if q[1]) >= 2, "solve %d: fewer than 2 accepted steps - the controller is not exercised" % k
    S.REPLAY = [list(q) for q in ref_seq]
    try:
        r64 = oracle_adjoint(L.odefunc, [p.adj], p.params, p.x0, R, torch.float64, method="dopri5", rtol=tol, atol=tol)
        assert S.REPLAY == []
    finally:
        S.REPLAY = None

    def run():
        p.f.zero_grad(set_to_none=True)
        x = p.x0.clone().requires_grad_(True)
        y = OI.odeint_adjoint(p.f, x, torch.tensor(T01, device=dev()), rtol=tol, atol=tol, method="dopri5")[1]
        (y * p.R).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), x.grad.clone(), [q.grad.clone() for q in p.f.parameters()]
    PS.TRACE = []
    try:
        run()
        got_seq = PS.TRACE
    finally:
        PS.TRACE = None
    PS.REPLAY = [list(q) for q in ref_seq]
    try:
        replayed = run()
        assert PS.REPLAY == []
    finally:
        PS.REPLAY = None
    check_vs_oracle(replayed, {torch.float32: r32, torch.float64: r64}, PNAMES, "dopri5 replayed")
    from test_gpu_gcn import _same_steps
    compared = _same_steps(got_seq, ref_seq, "2^17-row dopri5")
    assert compared[0] == len(ref_seq[0]) and compared[1] >= 2, (compared, [len(s) for s in ref_seq])


# ---------------------------------------------------------------------------------------------------------------------
# 4. one stage of the augmented field at the benchmark's size
# ---------------------------------------------------------------------------------------------------------------------
def test_adjoint_stage_at_benchmark_size_vs_autograd():
    """rmat_graph(20, 10 000 000), d = 128, node_order "auto" (renumbers at this size): k_y, k_a, a_t and the four
    parameter-gradient blocks of one evaluation of the augmented adjoint field (GcnOdeAdjointField.eval) against
    autograd through layers_ref.odefunc with cotangent -a, at the noise floor of fp32 vs fp64."""
    import gc
    from graph_odenet_amd import odeint as OI, synth
    from oracle import layers_ref as L
    g = synth.rmat_graph(20, 10_000_000, seed=0, device=dev())
    d, t = 128, 0.375
    f = make_func(d, g, seed=41, node_order="auto")
    torch.manual_seed(42)
    y = torch.randn(g.n_rows, d, device=dev())
    a = torch.randn(g.n_rows, d, device=dev())
    fwd, mk_adj, plist = OI._fields(f, y)
    order, inverse = fwd.row_order, fwd.row_inverse
    assert order is not None, "node_order='auto' must renumber the 2^20-row R-MAT graph"
    adj = mk_adj()
    yp, ap = y.index_select(0, order), a.index_select(0, order)
    out = adj._packed_like([yp, ap])
    with torch.no_grad():
        adj.eval(t, [[(1.0, yp)], [(1.0, ap)]], out)
    torch.cuda.synchronize()
    got = [out[0].index_select(0, inverse).cpu(), out[1].index_select(0, inverse).cpu(), out[2].cpu()]
    got += [q.cpu() for q in adj.param_grads(out)]
    assert [id(q) for q in plist] == [id(q) for q in f.parameters()]
    del out, yp, ap, fwd, adj, mk_adj
    A = cpu_coo(g)
    ycpu, acpu = y.cpu(), a.cpu()
    params = [q.detach().cpu() for q in f.parameters()]
    del f, g, y, a
    torch.cuda.empty_cache()
    names = ["k_y", "k_a", "a_t"] + ["dL/d" + k for k in PNAMES]

    def ref(dtype):
        tt = torch.tensor(t, dtype=dtype, requires_grad=True)
        x = ycpu.to(dtype).requires_grad_(True)
        ps = [q.to(dtype).requires_grad_(True) for q in params]
        fe = L.odefunc(tt, x, A.to(dtype), *ps)
        vj = torch.autograd.grad(fe, [x, tt] + ps, -acpu.to(dtype))
        return [fe.detach(), vj[0], vj[1].reshape(1)] + list(vj[2:])
    r32 = ref(torch.float32)
    gc.collect()
    r64 = ref(torch.float64)
    for k, u, v, w in zip(names, got, r32, r64):
        noise_floor_check(u, v, w, "2^20 rows " + k)
    del r32, r64
    gc.collect()


# ---------------------------------------------------------------------------------------------------------------------
# 5. GAT ODE fields above 65 536 nodes inside an adjoint solve
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gat_edges():
    n, per, hub = 70_001, 8, 3000
    g = torch.Generator().manual_seed(51)
    E = n * per
    src = torch.randint(0, n, (E + hub,), generator=g)
    tgt = torch.cat([torch.randint(0, n, (E,), generator=g), torch.full((hub,), 17, dtype=torch.int64)])
    Mtgt = torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(E + hub)]), torch.ones(E + hub), (n, E + hub))
    return n, src, tgt, Mtgt


@pytest.mark.parametrize("heads", [1, 4])
def test_gat_rk4_adjoint_large_vs_oracle(gat_edges, heads):
    """70 001 nodes, 8 edges per node plus a 3000-in-edge hub, rk4 step 0.5 on [0, 1] with the adjoint: the
    single-head ODEfunc at d = 16 against layers_ref.gat_odefunc, a 4-head field at d = 32 against the oracle heads;
    the fields run off the launch-bound / merged-reduction path."""
    from graph_odenet_amd import gat_heads, gat_models, gat_ode, models
    from oracle import layers_ref as L
    n, src, tgt, Mtgt = gat_edges
    torch.manual_seed(52 + heads)
    if heads == 1:
        d = 16
        f = gat_models.ODEfunc(d)
        names = ["norm1.weight", "norm1.bias", "gc1.f.weight", "gc1.f.bias", "gc1.w.weight", "gc1.w.bias"]

        def ofunc(tt, x, *ps):
            return L.gat_odefunc(tt, x, src, tgt, Mtgt.to(x.dtype), *ps)
    else:
        d = 32
        f = gat_heads.ODEfunc(d, heads)
        names = ["norm1.weight", "norm1.bias"] + ["gc1.heads.%d.%s" % (h, k) for h in range(heads)
                                                  for k in ("f.weight", "f.bias", "w.weight", "w.bias")]

        def ofunc(tt, x, *ps):
            hs = [list(ps[2 + 4 * h:6 + 4 * h]) for h in range(heads)]
            return L.gat_multihead_odefunc(tt, x, src, tgt, Mtgt.to(x.dtype), ps[0], ps[1], hs)
    with torch.no_grad():
        f.norm1.weight.uniform_(0.5, 1.5)
        f.norm1.bias.uniform_(-0.5, 0.5)
    pd = dict(f.named_parameters())
    assert sorted(pd) == sorted(names)
    params = [pd[k] for k in names]
    x0 = torch.randn(n, d) * 0.5
    R = torch.randn(n, d)
    ref = oracle_pair(ofunc, [], params, x0, R)
    f = f.to(dev())
    gr = (src.to(dev()), tgt.to(dev()), Mtgt.to(dev()))
    f.set_adj(*gr)
    fields = f.gode_fields(x0.to(dev()))
    assert fields is not None and getattr(fields[0], "fused", False)
    assert n > gat_ode.MERGED_FINISH_MAX_ROWS and not fields[0].small(), "GAT field on the launch-bound path"
    blk = models.ODEBlock(f, method="rk4", step_size=STEP)
    x = x0.to(dev()).requires_grad_(True)
    y = blk(x, *gr)
    (y * R.to(dev())).sum().backward()
    pd = dict(f.named_parameters())
    got = (y.detach(), x.grad, [pd[k].grad for k in names])
    check_vs_oracle(got, ref, names, "GAT H=%d" % heads)
