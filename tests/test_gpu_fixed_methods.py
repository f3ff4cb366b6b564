"""Fixed-grid euler and midpoint solves on the GPU - odeint (backprop through the solve), odeint_adjoint, the C drivers of the
GCN and GAT ODE functions, the edge-conditioned block, HIP-graph capture and nfe - against the float64 restatement of
tests/fixed_methods_ref.py run on the oracle's restatement of the same ODE function (oracle/layers_ref.py), on the CPU.

Yardstick: noise_floor_check (tests/test_gpu_gcn.py, copied into fixed_methods_ref) at its slack 4 - the error against
float64 at most 4 x the float32 restatement's own error + 1e-5 of the magnitude; forward results of one solve against the
float32 restatement at the plain 1e-5 close().  Graphs are random with self loops, n = 257 (no tile is full), 1 and 3 steps;
one large-route case (66 000 rows, d = 128)."""
import functools

import pytest
import torch

import fixed_methods_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
METHODS = ["euler", "midpoint"]
STEPS = [1, 3]
N = 257


def product_run(f, x0, t, Rw, method, step_size, adjoint, params=None):
    """odeint / odeint_adjoint of the product with L = sum_i <y(t_i), Rw_i> -> (outputs, dL/dx0, [dL/dparam], (nfe forward,
    nfe backward))."""
    from graph_odenet_amd import odeint as OI
    params = list(f.parameters()) if params is None else params
    for p in params:
        p.grad = None
    x = x0.detach().to(DEV).requires_grad_(True)
    if hasattr(f, "nfe"):
        f.nfe = 0
    solve = OI.odeint_adjoint if adjoint else OI.odeint
    out = solve(f, x, torch.tensor(t, device=DEV), method=method, options=None if step_size is None else {"step_size": step_size})
    assert out.grad_fn is not None
    nfe_f = getattr(f, "nfe", None)
    if nfe_f is not None:
        f.nfe = 0
    (out * Rw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), x.grad.clone(), [p.grad.clone() for p in params], (nfe_f, getattr(f, "nfe", None))


def check_all(got, refs, what, names, forward_close=True):
    (o32, gx32, gp32), (o64, gx64, gp64) = refs
    out, gx, gp = got[:3]
    if forward_close:
        R.close(out, o32, 1e-5, what + " y(t) vs fp32")
    else:
        print("%-44s err %.3e  (not asserted)" % (what + " y(t) vs fp32", (out.detach().cpu().double() - o32.double()).abs().max().item()))
    R.noise_floor_check(out, o32, o64, what + " y(t)")
    R.noise_floor_check(gx, gx32, gx64, what + " dL/dx0")
    assert len(gp) == len(gp64)
    for k, g, g32, g64 in zip(names, gp, gp32, gp64):
        R.noise_floor_check(g.reshape(g64.shape), g32, g64, what + " dL/d" + k)


def end_weights(shape, seed):
    """Cotangents for t = [0, 1]: zero on y(0), random on y(1)."""
    Rw = torch.zeros((2,) + tuple(shape))
    Rw[1] = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return Rw


# ---- the generic autograd field ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("n_steps", STEPS)
@pytest.mark.parametrize("method", METHODS)
def test_generic_autograd_field(method, n_steps, adjoint):
    """A two-layer tanh MLP as func (state 257 x 8): forward, and the gradients of y0 and the parameters through odeint
    (backprop) and through odeint_adjoint."""
    d = 8
    f = R.Mlp(d, seed=3).to(DEV)
    x0 = torch.randn(N, d, generator=torch.Generator().manual_seed(4))
    Rw = end_weights((N, d), 5)
    got = product_run(f, x0, [0.0, 1.0], Rw, method, 1.0 / n_steps, adjoint)
    refs = R.reference_runs(lambda dt: R.Mlp(d, seed=3).to(dt), x0, [0.0, 1.0], Rw, method, 1.0 / n_steps, adjoint)
    check_all(got, refs, "mlp %s n=%d %s" % (method, n_steps, "adjoint" if adjoint else "backprop"),
              [k for k, _ in f.named_parameters()])


# ---- the GCN ODE function ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gcn_adj(n=N, n_edges=1500, seed=11):
    return R.random_adj(n, n_edges, seed)


def gcn_func(d, adj, seed=0):
    from graph_odenet_amd import models
    torch.manual_seed(seed)
    f = models.ODEfunc(d)
    with torch.no_grad():
        f.norm1.weight.uniform_(0.5, 1.5)
        f.norm1.bias.uniform_(-0.5, 0.5)
    f = f.to(DEV)
    f.set_adj(adj.to(DEV))
    return f


def gcn_params(f):
    sd = dict(f.named_parameters())
    return [sd[k] for k in R.GCN_PNAMES]


@functools.lru_cache(maxsize=None)
def gcn_refs(d, method, n_steps, adjoint, times=(0.0, 1.0), every=False):
    """The float32 / float64 restatement runs of one GCN case, computed once and shared."""
    adj = gcn_adj()
    f = gcn_func(d, adj)
    x0, Rw = gcn_inputs(d, times, every)
    step = 1.0 / n_steps if isinstance(n_steps, int) else n_steps
    return R.reference_runs(lambda dt: R.GcnRef(f, adj, dt), x0, list(times), Rw, method, step, adjoint)


def gcn_inputs(d, times=(0.0, 1.0), every=False):
    x0 = torch.randn(N, d, generator=torch.Generator().manual_seed(6))
    if every:
        Rw = torch.randn((len(times), N, d), generator=torch.Generator().manual_seed(7))
    else:
        Rw = end_weights((N, d), 7)
    return x0, Rw


def gcn_block_run(d, method, n_steps, adjoint):
    """Through the public block: ODEBlock(method=, step_size=, adjoint=) -> (y(1), dL/dx, gradients in GCN_PNAMES order, nfe)."""
    from graph_odenet_amd import models
    adj = gcn_adj()
    f = gcn_func(d, adj)
    blk = models.ODEBlock(f, method=method, step_size=1.0 / n_steps, adjoint=adjoint)
    x0, Rw = gcn_inputs(d)
    x = x0.to(DEV).requires_grad_(True)
    f.nfe = 0
    y = blk(x, adj.to(DEV))
    nfe_f, f.nfe = f.nfe, 0
    (y * Rw[1].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach().clone(), x.grad.clone(), [p.grad.clone() for p in gcn_params(f)], (nfe_f, f.nfe)


def check_block(got, refs, what):
    """check_all for a block's y(1)."""
    (o32, gx32, gp32), (o64, gx64, gp64) = refs
    check_all(got, [(o32[1], gx32, gp32), (o64[1], gx64, gp64)], what, R.GCN_PNAMES)


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("n_steps", STEPS)
@pytest.mark.parametrize("d,small_fused", [(16, 1), (32, 1), (32, 0), (64, 1)])
@pytest.mark.parametrize("method", METHODS)
def test_gcn_block(method, d, small_fused, n_steps, adjoint):
    """ODEBlock on the GCN ODEfunc: forward, adjoint gradients (adjoint=True: the C drivers gode_gcn_ode_fixed_forward /
    _fixed_adjoint on the one-launch route, the per-stage driver behind the native forward elsewhere) and backprop gradients
    (adjoint=False: gode_gcn_ode_fixed_forward_save / _fixed_backprop).  d = 16, 32: the one-launch route; d = 32 with
    option small_fused 0, and d = 64: the multi-launch route.  nfe: S n after the forward; S n + 1 after an adjoint backward
    (the counted-but-skipped dL/dt evaluation), 0 after a backprop backward."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    old = lib.gode_get_option(b"small_fused")
    lib.gode_set_option(b"small_fused", small_fused)
    try:
        got = gcn_block_run(d, method, n_steps, adjoint)
    finally:
        lib.gode_set_option(b"small_fused", old)
    what = "gcn %s d=%d sf=%d n=%d %s" % (method, d, small_fused, n_steps, "adjoint" if adjoint else "backprop")
    check_block(got, gcn_refs(d, method, n_steps, adjoint), what)
    S = R.STAGES[method]
    assert got[3] == (S * n_steps, S * n_steps + 1 if adjoint else 0), got[3]


@pytest.mark.parametrize("method", METHODS)
def test_gcn_large_route(method):
    """66 000 rows, d = 128, about 200 000 edges, 2 steps: the large-route launches of the forward driver, the per-stage adjoint
    (gode_gcn_ode_fixed_adjoint refuses the size) and the multi-launch backprop sweep.

    Backprop differentiates the computed solution, relu's branch included, and of the 1.7e7 pre-activations of this case one
    lies 1.5e-8 (euler) / 2.4e-8 (midpoint) from the kink in float64, where the fp32 solve takes the other branch (measured:
    against plain float64 dL/dx0 is off by 2.5e-2 / 1.2e-3, with that one branch prescribed by 1.8e-4 / 1.9e-4, the float32
    restatement's own error being 5.1e-4).  So the backprop leg's restatement takes the branch the records of the solve show
    wherever |z| < 1e-5 (fixed_methods_ref.GcnRefBranch), and the test asserts that outside that band the recorded branches
    are float64's."""
    from graph_odenet_amd import models
    n, d = 66000, 128
    adj = R.random_adj(n, 134000, 13)
    f = gcn_func(d, adj, seed=2)
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(8))
    Rw = end_weights((n, d), 9)
    for adjoint in (True, False):
        blk = models.ODEBlock(f, method=method, step_size=0.5, adjoint=adjoint)
        f.zero_grad(set_to_none=True)
        x = x0.to(DEV).requires_grad_(True)
        y = blk(x, adj.to(DEV))
        (y * Rw[1].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        got = (y.detach(), x.grad, [p.grad for p in gcn_params(f)])
        made = []
        if adjoint:
            mk = lambda dt: R.GcnRef(f, adj, dt)      # noqa: E731
        else:
            S = R.STAGES[method]
            fwd = f.gode_fields(x0.to(DEV))[0]
            rec = torch.empty((2, S + 1, n, d), device=DEV)
            rec[0, 0].copy_(x0)
            fwd.fixed_forward_save(method, rec[0, 0], torch.empty(n, d, device=DEV), rec, 0.0, 1.0, 2, 0, 2)
            branches = [(rec[i, 1 + s] > 0).cpu() for i in range(2) for s in range(S)]

            def mk(dt):
                made.append(R.GcnRefBranch(f, adj, dt, branches))
                return made[-1]
        refs = R.reference_runs(mk, x0, [0.0, 1.0], Rw, method, 0.5, adjoint)
        for ref in made:
            print("branches taken from the solve within 1e-5 of the kink: %d; differing outside: %d" % (ref.near, ref.disagree))
            assert ref.disagree == 0 and not ref.branches
        check_block(got, refs, "gcn large %s %s" % (method, "adjoint" if adjoint else "backprop"))


@pytest.mark.parametrize("method", METHODS)
def test_gcn_native_against_per_stage(method, monkeypatch):
    """With odeint.NATIVE_RK4 = False the same solves run through solver.integrate_fixed and the generic backprop path: inside
    the yardstick as well (whether they are bit for bit the native ones is printed, not demanded)."""
    from graph_odenet_amd import odeint as OI
    d, n_steps = 16, 3
    native = {adj: gcn_block_run(d, method, n_steps, adj) for adj in (True, False)}
    monkeypatch.setattr(OI, "NATIVE_RK4", False)
    for adjoint in (True, False):
        got = gcn_block_run(d, method, n_steps, adjoint)
        what = "gcn per-stage %s %s" % (method, "adjoint" if adjoint else "backprop")
        check_block(got, gcn_refs(d, method, n_steps, adjoint), what)
        same = torch.equal(got[0], native[adjoint][0]) and torch.equal(got[1], native[adjoint][1]) and \
            all(torch.equal(a, b) for a, b in zip(got[2], native[adjoint][2]))
        print("%s: bit-equal to the native path: %s" % (what, same))


def test_gcn_three_output_times():
    """t = [0, 0.4, 1.0] with a cotangent on every output (d = 16, midpoint, step_size 0.2: 2 and 3 steps): outputs and
    gradients through odeint (backprop) and odeint_adjoint."""
    d, times = 16, (0.0, 0.4, 1.0)
    f = gcn_func(d, gcn_adj())
    x0, Rw = gcn_inputs(d, times, True)
    for adjoint in (False, True):
        got = product_run(f, x0, list(times), Rw, "midpoint", 0.2, adjoint, params=gcn_params(f))
        refs = gcn_refs(d, "midpoint", 0.2, adjoint, times, True)
        assert torch.equal(got[0][0].cpu(), x0)
        check_all(got, refs, "gcn 3 times %s" % ("adjoint" if adjoint else "backprop"), R.GCN_PNAMES)


# ---- the GAT ODE function ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gat_edges():
    return R.random_edges(N, 1200, 17)


def gat_func(d, H, seed=5):
    from graph_odenet_amd import gat_heads, gat_models
    src, tgt = gat_edges()
    torch.manual_seed(seed)
    f = gat_models.ODEfunc(d) if H == 1 else gat_heads.ODEfunc(d, H)
    with torch.no_grad():
        f.norm1.weight.add_(0.3 * torch.randn(d))
        f.norm1.bias.add_(0.3 * torch.randn(d))
    f = f.to(DEV)
    f.set_adj(src.to(DEV), tgt.to(DEV), R.mtgt(N, tgt).to(DEV))
    return f


@pytest.mark.parametrize("n_steps", STEPS)
@pytest.mark.parametrize("d,H", [(16, 1), (32, 4)])
@pytest.mark.parametrize("method", METHODS)
def test_gat(method, d, H, n_steps):
    """Forward and adjoint through the per-stage driver (solver.integrate_fixed, the small components closed once per step);
    backprop through gode_gat_ode_fixed_forward_save / _fixed_backprop, also against the generic path (BACKPROP_FUSED off)
    at 1e-4.

    The outputs are held to the noise floor against float64 and not to the 1e-5 close() against the float32 restatement:
    on this function the float32 restatement itself is 1.1e-5 .. 1.9e-5 from float64 (scale 1.8 .. 2.2; the softmax over
    the in-edges) and the solve under test 1.2e-5 .. 1.9e-5, so the two float32 results are 1.6e-5 .. 2.7e-5 apart over the
    eight cases (printed, not asserted)."""
    from graph_odenet_amd import gat_ode
    src, tgt = gat_edges()
    f = gat_func(d, H)
    x0 = 0.5 * torch.randn(N, d, generator=torch.Generator().manual_seed(9))
    Rw = end_weights((N, d), 10)
    names = [k for k, _ in f.named_parameters()]
    mk = lambda dt: R.GatRef(f, N, src, tgt, dt)      # noqa: E731
    fwd = f.gode_fields(x0.to(DEV))[0]
    assert fwd.fixed_forward_save is not None and fwd.fixed_backprop is not None
    what = "gat %s d=%d H=%d n=%d " % (method, d, H, n_steps)
    for adjoint in (True, False):
        got = product_run(f, x0, [0.0, 1.0], Rw, method, 1.0 / n_steps, adjoint)
        refs = R.reference_runs(mk, x0, [0.0, 1.0], Rw, method, 1.0 / n_steps, adjoint)
        check_all(got, refs, what + ("adjoint" if adjoint else "backprop"), names, forward_close=False)
        S = R.STAGES[method]
        assert got[3] == (S * n_steps, S * n_steps + 1 if adjoint else 0), got[3]
    gat_ode.GatOdeField.BACKPROP_FUSED = False
    try:
        assert f.gode_fields(x0.to(DEV))[0].fixed_forward_save is None
        generic = product_run(f, x0, [0.0, 1.0], Rw, method, 1.0 / n_steps, False)
    finally:
        gat_ode.GatOdeField.BACKPROP_FUSED = True
    R.close(got[0], generic[0], 1e-4, what + "fused vs generic y")
    R.close(got[1], generic[1], 1e-4, what + "fused vs generic dL/dx0")
    for k, a, b in zip(names, got[2], generic[2]):
        R.close(a, b, 1e-4, what + "fused vs generic dL/d" + k)


# ---- the edge-conditioned block ------------------------------------------------------------------------------------------------
EDGE_KEYS = ("gamma", "beta", "W", "b", "A")
EDGE_DRAWS = 6


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("method", METHODS)
def test_edge_block(method, adjoint):
    """EdgeODEBlock at the shapes of tests/test_gpu_edge_backprop.py (batch_of(20, 96, seed=7), step 0.25): forward, adjoint
    and backprop (the Python sweeps of qc_ode.EdgeOdeField over S stages), the edge matrices' gradient included.

    The yardstick's figure "the float32 restatement's own error" is here the largest over EDGE_DRAWS = 6 float32 evaluations
    of the case, not one: the case itself and five copies whose start state is moved by one float32 rounding (relative
    6e-8), each against float64 on the same inputs.  Measured: GroupNorm(32, 96) has three channels per group and its
    backward amplifies rounding by 1 / spread of a triple, so one draw of that error is anywhere in a range of 13 x - on the
    euler backprop leg dL/db 3.0e-4 .. 3.8e-3 and dL/dx0 7.4e-4 .. 7.6e-3 over the six, the case's own draw 5.9e-4 and
    9.5e-4 - while the solve under test sits at 3.0e-3 and 5.5e-3, inside that range, with every relu branch it recorded
    equal to float64's.  Against its own single draw that leg misses slack 4 (dL/dx0 5.5e-3 against 4 x 9.5e-4 + 9.3e-4).
    The outputs keep the single figure and the plain 1e-5 close()."""
    from test_gpu_qc_ode import batch_of, block_run, product
    h = 96
    x0, Esrc, etgt, val, A, _ = batch_of(20, h, seed=7)
    f, Ad = product(h, Esrc, etgt, val, A)
    Rw = end_weights(x0.shape, 4)
    got, nfe = block_run(f, Ad, x0, Rw[1], method, 0.25, adjoint=adjoint)
    ((o32, gx32, gp32), (o64, gx64, gp64)), worst = edge_refs(method, adjoint)
    what = "edge %s %s" % (method, "adjoint" if adjoint else "backprop")
    R.close(got["y"], o32[1], 1e-5, what + " y(1) vs fp32")
    R.noise_floor_check(got["y"], o32[1], o64[1], what + " y(1)")
    R.noise_floor_check(got["x"], gx32, gx64, what + " dL/dx0", e_ref_draws=worst[0])
    for i, k in enumerate(EDGE_KEYS):
        R.noise_floor_check(got[k], gp32[i], gp64[i], what + " dL/d" + k, e_ref_draws=worst[1 + i])
    S = R.STAGES[method]
    assert nfe == (4 * S, 4 * S + 1 if adjoint else 0), nfe


@functools.lru_cache(maxsize=None)
def edge_refs(method, adjoint):
    """(the float32 / float64 restatement runs of the edge case, the largest float32-against-float64 error of dL/dx0 and of
    each gradient in EDGE_KEYS order over EDGE_DRAWS draws: the case, and copies with x0 moved by one float32 rounding)."""
    from test_gpu_qc_ode import batch_of
    from test_qc_ode_api import RefEdgeODEfunc, randomise
    from graph_odenet_amd import qc_ode
    h = 96
    x0, Esrc, etgt, val, A, _ = batch_of(20, h, seed=7)
    torch.manual_seed(5)                                   # test_gpu_qc_ode.product's parameters
    f = randomise(qc_ode.EdgeODEfunc(h))
    Rw = end_weights(x0.shape, 4)
    first, worst = None, None
    for draw in range(EDGE_DRAWS):
        g = torch.Generator().manual_seed(100 + draw)
        xp = x0 if draw == 0 else (x0 * (1 + 6e-8 * torch.randn(x0.shape, generator=g))).float()
        pair = {dt: RefEdgeODEfunc(h, Esrc, etgt, val, A, dtype=dt).load(f) for dt in (torch.float32, torch.float64)}
        refs = R.reference_runs(lambda dt: pair[dt], xp, [0.0, 1.0], Rw, method, 0.25, adjoint,
                                params_of=lambda r: [getattr(r, k) for k in EDGE_KEYS])
        (_, gx32, gp32), (_, gx64, gp64) = refs
        errs = [(gx32.double() - gx64).abs().max().item()] + [(a.double() - b).abs().max().item() for a, b in zip(gp32, gp64)]
        first = refs if draw == 0 else first
        worst = errs if worst is None else [max(u, v) for u, v in zip(worst, errs)]
    return first, worst


# ---- the re-run mode of backprop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gcn", "gat"])
@pytest.mark.parametrize("method", METHODS)
def test_rerun_mode_bit_identical(method, kind, monkeypatch):
    """With BACKPROP_SAVE_MAX_BYTES = 0 only y_n is kept and each step re-run into a one-step record before its sweep: the
    gradients of a 3-step solve are bit for bit those of the save-everything mode."""
    from graph_odenet_amd import odeint as OI
    d = 16
    f = gcn_func(d, gcn_adj()) if kind == "gcn" else gat_func(d, 1)
    x0 = 0.5 * torch.randn(N, d, generator=torch.Generator().manual_seed(12))
    Rw = end_weights((N, d), 13)
    assert f.gode_fields(x0.to(DEV))[0].fixed_forward_save is not None
    full = product_run(f, x0, [0.0, 1.0], Rw, method, 1 / 3, False)
    monkeypatch.setattr(OI, "BACKPROP_SAVE_MAX_BYTES", 0)
    rerun = product_run(f, x0, [0.0, 1.0], Rw, method, 1 / 3, False)
    assert torch.equal(full[0], rerun[0]) and torch.equal(full[1], rerun[1])
    for a, b in zip(full[2], rerun[2]):
        assert torch.equal(a, b)


# ---- capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_capture_and_replay(method):
    """The same block called three times: the second call captures the solves, the third replays them; results and gradients
    are bit for bit the first (eager) call's."""
    from graph_odenet_amd import models, odeint as OI
    d = 16
    adj = gcn_adj()
    f = gcn_func(d, adj)
    blk = models.ODEBlock(f, method=method, step_size=1 / 3)
    x0, Rw = gcn_inputs(d)
    adj_dev = adj.to(DEV)
    runs = []
    for _ in range(3):
        f.zero_grad(set_to_none=True)
        x = x0.to(DEV).requires_grad_(True)
        y = blk(x, adj_dev)
        (y * Rw[1].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in gcn_params(f)])
    plans = list(OI.plans_of(f).values())
    assert len(plans) == 1 and plans[0].gf is not None and plans[0].gb is not None and not plans[0].no_capture
    assert plans[0].gf.nfe == R.STAGES[method] * 3
    for later in runs[1:]:
        for a, b in zip(runs[0], later):
            assert torch.equal(a, b)


def test_capture_plans_are_keyed_by_method(monkeypatch):
    """On one func: an rk4 solve, an euler solve and an rk4 solve again, each requested often enough to be captured - every
    one equals its own eager result (without the method in the plan key the euler solve would replay the rk4 graph)."""
    from graph_odenet_amd import odeint as OI
    d = 16
    f = gcn_func(d, gcn_adj())
    x = gcn_inputs(d)[0].to(DEV)
    t = torch.tensor([0.0, 1.0], device=DEV)

    def solve(method):
        with torch.no_grad():
            return OI.odeint_adjoint(f, x, t, method=method, options={"step_size": 0.5})[1].clone()
    monkeypatch.setattr(OI, "GRAPH_CAPTURE_MAX_ELEMS", 0)
    eager = {m: solve(m) for m in ("rk4", "euler", "midpoint")}
    assert not OI.plans_of(f)
    assert not torch.equal(eager["rk4"], eager["euler"]) and not torch.equal(eager["midpoint"], eager["euler"])
    monkeypatch.setattr(OI, "GRAPH_CAPTURE_MAX_ELEMS", 1 << 21)
    for m in ("rk4", "rk4", "euler", "euler", "rk4", "midpoint", "midpoint", "euler", "rk4"):
        assert torch.equal(solve(m), eager[m]), m
    plans = OI.plans_of(f)
    assert len(plans) == 3 and all(p.gf is not None for p in plans.values())
    assert sorted(p.method for p in plans.values()) == ["euler", "midpoint", "rk4"]
