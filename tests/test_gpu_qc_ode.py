"""The continuous-depth edge-conditioned block (qc_ode.py, csrc/edge_ode.hip) on the GPU against the plain-torch
restatement of tests/test_qc_ode_api.py run on the CPU in float32 and float64, through oracle/solver_ref (unchanged).

Bars: noise_floor_check of tests/test_gpu_gcn.py (error against float64 within slack x the float32 restatement's own
error + 1e-5 x scale); slack 4, and 20 at h = 16, where GroupNorm(16, 16) normalises single channels (the documented
degeneracy, tests/test_gpu_gcn.py)."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_gcn import _same_steps, noise_floor_check
from test_gpu_large_adjoint import profiled
from test_qc_ode_api import RefEdgeODEfunc, randomise

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def slack_of(h):
    return 20.0 if h == 16 else 4.0


def batch_of(n_graphs, h, seed):
    """Seeded QM9-like batch as index vectors, with an atom that is no edge's target, a duplicated (src, tgt) pair and
    non-unit Etgt values.  Returns CPU tensors: x0 (N x h), Esrc, etgt, val, A (E x h x h), and the loader's
    (node features, edge features, batch)."""
    from graph_odenet_amd.synth import qm9_like_batch
    xf, ef, Esrc, Etgt, batch = qm9_like_batch(n_graphs, seed=seed)
    etgt = Etgt.argmax(0)
    u = Etgt.shape[0] - 1
    etgt[etgt == u] = u - 1                         # the last atom receives nothing
    Esrc = Esrc.clone()
    Esrc[1], etgt[1] = Esrc[0], etgt[0]             # a duplicated pair
    g = torch.Generator().manual_seed(seed + 100)
    val = torch.rand(Esrc.numel(), generator=g) + 0.5
    A = torch.randn(Esrc.numel(), h, h, generator=g) * (0.5 / h ** 0.5)
    x0 = torch.randn(Etgt.shape[0], h, generator=g)
    return x0, Esrc, etgt, val, A, (xf, ef, batch)


def dense_etgt(n, etgt, val):
    M = torch.zeros(n, etgt.numel())
    M[etgt, torch.arange(etgt.numel())] = val
    return M


def product(h, Esrc, etgt, val, A, form="prepared"):
    from graph_odenet_amd import qc_layers, qc_ode
    torch.manual_seed(5)
    f = randomise(qc_ode.EdgeODEfunc(h)).to(DEV)
    n = int(etgt.max()) + 2
    Etgt = qc_layers.prepared_edges(Esrc.to(DEV), etgt.to(DEV), n, val.to(DEV)) if form == "prepared" else \
        dense_etgt(n, etgt, val).to(DEV)
    Ad = A.to(DEV).requires_grad_(True)
    f.set_edges(Esrc.to(DEV), Etgt, Ad)
    return f, Ad


NAMES = ("gamma", "beta", "W", "b", "A")
PNAMES = {"gamma": "norm1.weight", "beta": "norm1.bias", "W": "gc1.weight", "b": "gc1.bias"}


def ref_pair(f, h, Esrc, etgt, val, A):
    return [RefEdgeODEfunc(h, Esrc, etgt, val, A, dtype=dt).load(f) for dt in (torch.float32, torch.float64)]


@pytest.mark.parametrize("h,n_graphs", [(16, 20), (64, 20), (96, 20), (64, 120)])
def test_one_evaluation_and_vjp_through_the_fused_fields(h, n_graphs):
    from graph_odenet_amd import ops
    x0, Esrc, etgt, val, A, _ = batch_of(n_graphs, h, seed=1)
    assert (Esrc.numel() >= ops.EDGE_ODE_FUSED_MAX_EDGES) == (n_graphs == 120)
    f, Ad = product(h, Esrc, etgt, val, A)
    fields = f.gode_fields(x0.to(DEV))
    assert fields is not None
    fwd, mk_adj, plist = fields
    t = 0.375
    a = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9))
    x, ad = x0.to(DEV), a.to(DEV)
    out = torch.empty_like(x)
    with profiled() as kinds:
        fwd.eval(t, [[(1.0, x)]], [out])
    if n_graphs == 20:
        assert kinds.count(ops.PROF_EDGE_FEVAL) == 1
    else:
        assert ops.PROF_EDGE_FEVAL not in kinds
    adj = mk_adj()
    state = adj.new_state(x)
    k = adj.alloc_like(state, 1)[0]
    adj.eval(t, [[(1.0, x)], [(1.0, ad)], [(1.0, state[2])], [(1.0, state[3])], [(1.0, state[4])]], k)
    v = adj.s.views(k[3])
    got = {"f": out, "fy": k[0], "dx": k[1], "a_t": k[2], "gamma": v["gamma"], "beta": v["beta"], "W": v["W"], "b": v["b"], "A": k[4]}
    want = []
    for ref in ref_pair(f, h, Esrc, etgt, val, A):
        dt = ref.W.dtype
        tt = torch.tensor(t, dtype=dt, requires_grad=True)
        xr = x0.detach().clone().to(dt).requires_grad_(True)
        fe = ref(tt, xr)
        g = torch.autograd.grad(fe, (tt, xr, ref.gamma, ref.beta, ref.W, ref.b, ref.A), -a.to(dt))
        want.append(dict(zip(("f", "fy", "a_t", "dx", "gamma", "beta", "W", "b", "A"), (fe.detach(), fe.detach()) + g)))
    for key in got:
        noise_floor_check(got[key].reshape(want[1][key].shape), want[0][key], want[1][key], "h=%d %s" % (h, key), slack=slack_of(h))


def block_run(f, Ad, x0, R, method, step_size, tol=1e-5, adjoint=True):
    from graph_odenet_amd import qc_ode
    blk = qc_ode.EdgeODEBlock(f, tol=tol, method=method, step_size=step_size, adjoint=adjoint)
    f.zero_grad(set_to_none=True)
    Ad.grad = None
    x = x0.to(DEV).requires_grad_(True)
    f.nfe = 0
    y = blk(x, f.Esrc, f.Etgt, Ad)
    nfe_f = f.nfe
    f.nfe = 0
    (y * R.to(DEV)).sum().backward()
    g = {k: f.state_dict(keep_vars=True)[PNAMES[k]].grad.clone() for k in PNAMES}
    g.update(A=Ad.grad.clone(), x=x.grad.clone(), y=y.detach().clone())
    return g, (nfe_f, f.nfe)


def oracle_run(ref, x0, R, method, step_size, tol=1e-5):
    from oracle import solver_ref as S
    dt = ref.W.dtype
    ref.zero_grad(set_to_none=True)
    ref.nfe = 0
    x = x0.detach().clone().to(dt).requires_grad_(True)
    opts = None if step_size is None else {"step_size": step_size}
    y = S.odeint_adjoint(ref, x, torch.tensor([0.0, 1.0], dtype=dt), rtol=tol, atol=tol, method=method, options=opts)[1]
    nfe_f = ref.nfe
    ref.nfe = 0
    (y * R.to(dt)).sum().backward()
    g = {k: getattr(ref, k).grad.clone() for k in NAMES}
    g.update(x=x.grad.clone(), y=y.detach().clone())
    return g, (nfe_f, ref.nfe)


@pytest.mark.parametrize("h", [16, 64])
def test_block_rk4_adjoint_vs_oracle_fused_and_generic(h):
    """EdgeODEBlock under rk4 (4 steps): y(1), dL/dx, the parameter gradients and dL/d(edge_data) against the oracle's
    adjoint over the restatement - through the fused fields, through the generic autograd fields of the same module
    (hook switched off), and with the per-step edge-matrix pass forced off; nfe as the oracle counts it."""
    from graph_odenet_amd import ops, qc_ode
    x0, Esrc, etgt, val, A, _ = batch_of(20, h, seed=2)
    R = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4))
    f, Ad = product(h, Esrc, etgt, val, A, form="dense")
    (g32, nfe32), (g64, _) = [oracle_run(r, x0, R, "rk4", 0.25) for r in ref_pair(f, h, Esrc, etgt, val, A)]
    with profiled() as kinds:
        got, nfe = block_run(f, Ad, x0, R, "rk4", 0.25)
    assert nfe == nfe32
    # the default route: one outer-sum pass per RK step, no stage forms its own dA
    assert kinds.count(ops.PROF_EDGE_OUTER_STEP) == 4 and ops.PROF_EDGE_OUTER_STAGE not in kinds
    assert kinds.count(ops.PROF_EDGE_VJP) == 16 and kinds.count(ops.PROF_EDGE_FEVAL) == 32
    again, _ = block_run(f, Ad, x0, R, "rk4", 0.25)
    for k in got:
        noise_floor_check(got[k], g32[k], g64[k], "fused h=%d %s" % (h, k), slack=slack_of(h))
        assert torch.equal(got[k], again[k]), "not deterministic: " + k
    qc_ode.EdgeOdeAdjointField.DEFER_EDGE_GRAD = False
    try:
        with profiled() as kinds:
            per_stage, _ = block_run(f, Ad, x0, R, "rk4", 0.25)
    finally:
        qc_ode.EdgeOdeAdjointField.DEFER_EDGE_GRAD = True
    assert kinds.count(ops.PROF_EDGE_OUTER_STAGE) == 16 and ops.PROF_EDGE_OUTER_STEP not in kinds
    for k in got:                      # another summation order, the same noise floor
        noise_floor_check(per_stage[k], g32[k], g64[k], "per-stage dA h=%d %s" % (h, k), slack=slack_of(h))
    qc_ode.EdgeODEfunc.FUSED = False
    try:
        assert f.gode_fields(x0.to(DEV)) is None
        generic, nfe_g = block_run(f, Ad, x0, R, "rk4", 0.25)
    finally:
        qc_ode.EdgeODEfunc.FUSED = True
    assert nfe_g == nfe32
    for k in got:
        noise_floor_check(generic[k], g32[k], g64[k], "generic h=%d %s" % (h, k), slack=slack_of(h))


def test_launches_per_evaluation_and_per_vjp():
    """Launch-bound batch, h = 64: an evaluation is 2 launches (<= 3), the VJP part of an adjoint stage 4 + a quarter of the
    per-step outer-sum pass (<= 8).  Counted from the profile kinds; gode_reduce_segments_f32, which the profile does not
    bracket, is counted by its calls."""
    from graph_odenet_amd import ops
    h = 64
    x0, Esrc, etgt, val, A, _ = batch_of(20, h, seed=3)
    f, Ad = product(h, Esrc, etgt, val, A)
    R = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4))
    calls = []
    orig = ops.reduce_segments_
    ops.reduce_segments_ = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        with profiled() as kinds:
            block_run(f, Ad, x0, R, "rk4", 0.25)
    finally:
        ops.reduce_segments_ = orig
    n_eval, n_stage = 32, 16                                     # 16 forward + 16 re-evaluations; 16 adjoint stages
    fam = [k & 0xff for k in kinds]
    evals = fam.count(ops.PROF_EDGE_FEVAL) + fam.count(1)        # GODE_PROF_GEMM_FWD
    vjp = fam.count(ops.PROF_EDGE_VJP) + fam.count(2) + fam.count(3) + len(calls) + fam.count(ops.PROF_EDGE_OUTER_STEP)
    assert len(fam) == evals + vjp - len(calls), "an unexpected kind of launch: %s" % sorted(set(fam))
    assert evals == 2 * n_eval and evals / n_eval <= 3
    assert vjp == 4 * n_stage + n_stage // 4 and vjp / n_stage <= 8


def test_block_dopri5_replayed_and_free_running_vs_oracle():
    """dopri5 at rtol = atol = 1e-5, h = 64, forward and adjoint.  Replaying the oracle's step sequence on the product's
    kernels: nfe equal to the oracle's and every gradient (dx, parameters, d(edge_data)) at the float32 noise floor.
    Free-running: the accept / reject walk against the oracle's (solver.TRACE).

    Free-running y(1): the product's own controller leaves the oracle's grid after some tens of attempts (float32
    rounding of the error estimate), and two adaptive runs on different grids are as far apart as the grid is worth.  The
    yardstick is that of free_running_check in tests/test_gpu_gcn.py, built from the oracle alone: the float64 oracle at
    tolerance 1e-5 against the float64 oracle at 1e-6 (discretisation) plus the float32 oracle's distance from the
    float64 replay of its own steps (rounding); |product - float64 oracle(1e-6)| <= 4 x (their sum) + 1e-5 x scale.
    (The state of this seeded problem grows from magnitude 1 to 15 over [0, 1], so both terms are far above 1e-5.)"""
    from graph_odenet_amd import solver as PS
    from oracle import solver_ref as S
    h = 64
    x0, Esrc, etgt, val, A, _ = batch_of(20, h, seed=6)
    R = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4))
    f, Ad = product(h, Esrc, etgt, val, A)
    r32, r64 = ref_pair(f, h, Esrc, etgt, val, A)
    S.TRACE = []
    try:
        g32, nfe32 = oracle_run(r32, x0, R, None, None)
        ref_seq = S.TRACE
    finally:
        S.TRACE = None
    S.REPLAY = [list(q) for q in ref_seq]
    try:
        g64, _ = oracle_run(r64, x0, R, None, None)
        assert S.REPLAY == []
    finally:
        S.REPLAY = None
    PS.TRACE = []
    try:
        free, nfe = block_run(f, Ad, x0, R, None, None)
        got_seq = PS.TRACE
    finally:
        PS.TRACE = None
    compared = _same_steps(got_seq, ref_seq, "edge ode dopri5")
    for k in (0, 1):                   # the attempts around the end of the common walk, before anything is asserted
        c = compared[k]
        print("solve %d: walked %d of %d / %d" % (k, c, len(got_seq[k]), len(ref_seq[k])), got_seq[k][max(c - 1, 0):c + 2],
              ref_seq[k][max(c - 1, 0):c + 2])
    # _same_steps itself fails on a forward decision that differs away from a tie.  How far the STEP SIZES can be asked to
    # agree follows from the number formats: at rtol = atol = 1e-5 on a state of magnitude 1 the float32 error estimate
    # (a difference of order 1e-6) carries rounding of order 6e-8 per element, i.e. percents of itself, so the next step
    # (ratio^-1/10) moves by parts in 1e3 per attempt and leaves _same_steps' 2e-3 window within tens of attempts: the
    # initial step and the first eight attempts (the controller before that noise accumulates) are demanded forward, the
    # initial step of the adjoint solve backward; everything after is covered by the replayed comparison below.
    assert compared[0] >= 8 and compared[1] >= 1
    # free-running: each side counts 2 evaluations for the initial step and 6 per attempt of ITS OWN walk (the counters of
    # the same walk are compared in the replayed run below)
    assert nfe[0] == 2 + 6 * len(got_seq[0]) and nfe32[0] == 2 + 6 * len(ref_seq[0])
    PS.REPLAY = [list(q) for q in ref_seq]
    try:
        rep, nfe_r = block_run(f, Ad, x0, R, None, None)
        assert PS.REPLAY == []
    finally:
        PS.REPLAY = None
    assert nfe_r == nfe32
    for k in rep:
        noise_floor_check(rep[k], g32[k], g64[k], "dopri5 replayed " + k)
    tt = torch.tensor([0.0, 1.0], dtype=torch.float64)
    with torch.no_grad():
        y5 = S.odeint(r64, x0.double(), tt, rtol=1e-5, atol=1e-5)[1]
        y6 = S.odeint(r64, x0.double(), tt, rtol=1e-6, atol=1e-6)[1]
    e_disc = (y5 - y6).abs().max().item()
    e_round = (g32["y"].double() - g64["y"]).abs().max().item()
    e_got = (free["y"].cpu().double() - y6).abs().max().item()
    scale = max(1.0, y6.abs().max().item())
    print("free-running y(1): err %.3e, discretisation %.3e, rounding %.3e, scale %.2e" % (e_got, e_disc, e_round, scale))
    assert e_got <= 4.0 * (e_disc + e_round) + 1e-5 * scale, \
        "free-running y(1): err %.3e vs discretisation %.3e + rounding %.3e" % (e_got, e_disc, e_round)


def test_block_backprop_through_rk4_vs_unrolled_autograd():
    """adjoint=False under rk4: gradients of the discrete solution = autograd through the restatement's rk4_38_step."""
    from oracle import solver_ref as S
    h = 64
    x0, Esrc, etgt, val, A, _ = batch_of(20, h, seed=7)
    R = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4))
    f, Ad = product(h, Esrc, etgt, val, A)
    want = []
    for ref in ref_pair(f, h, Esrc, etgt, val, A):
        dt = ref.W.dtype
        x = x0.detach().clone().to(dt).requires_grad_(True)
        y = x
        for i in range(4):
            y = y + S.rk4_38_step(lambda t, yy: (ref(t, yy[0]),), torch.tensor(0.25 * i, dtype=dt), torch.tensor(0.25, dtype=dt), (y,))[0]
        g = torch.autograd.grad((y * R.to(dt)).sum(), (ref.gamma, ref.beta, ref.W, ref.b, ref.A, x))
        want.append(dict(zip(NAMES + ("x",), g), y=y.detach()))
    got, _ = block_run(f, Ad, x0, R, "rk4", 0.25, adjoint=False)
    for k in got:
        noise_floor_check(got[k], want[0][k], want[1][k], "backprop " + k)


def _ref_model(p, name, ref_func, x, ef, Esrc, Etgt, batch, n_graphs, hidden):
    """The model on the CPU from oracle/models_ref's pieces and the restatement; returns (output, A, ode function)."""
    from oracle import layers_ref as L
    from oracle import models_ref as M
    from oracle import solver_ref as S
    A = M.edge_encoder(p, ef, hidden)
    hcur = F.relu(L.edge_graph_convolution(M._mlp2(p, "mlpin.mlp.", x), Esrc, Etgt, A, p["gcin.weight"], p["gcin.bias"]))
    ref_func.A = torch.nn.Parameter(A.detach().clone())
    hcur = S.odeint_adjoint(ref_func, hcur, torch.tensor([0.0, 1.0]), rtol=1e-5, atol=1e-5, method="rk4",
                            options={"step_size": 0.25})[1]
    hcur = L.edge_graph_convolution(hcur, Esrc, Etgt, A, p["gcout.weight"], p["gcout.bias"])
    if name.endswith("Set2Set"):
        q = L.set2set(hcur, batch, n_graphs, p["s2s.lstm.weight_ih_l0"], p["s2s.lstm.weight_hh_l0"], p["s2s.lstm.bias_ih_l0"],
                      p["s2s.lstm.bias_hh_l0"], 3)[:, :hidden]
        return M._mlp2(p, "mlpout.mlp.", q), A
    hcur = M._mlp2(p, "mlpout.mlp.", hcur)
    return torch.zeros(n_graphs, hcur.shape[1]).index_add_(0, batch, hcur), A


@pytest.mark.parametrize("name,mode", [("EdgeODE1_K_Sum", "eager"), ("EdgeODE1_K_Set2Set", "prepared")])
def test_models_train_like_the_cpu_reference(name, mode):
    """Five Adam steps (lr 1e-3, MSE) through qc_train.TrainStep, a new batch each step, against the same model built from
    the restatement and oracle.solver_ref.odeint_adjoint with torch.optim.Adam; tolerance of
    tests/test_gpu_harness.py::test_qc_training_trajectory_matches_reference (5e-5 x max(1, largest loss)).
    The batches carry non-unit Etgt values: "prepared" mode must hand them to the layers as "eager" mode does."""
    from graph_odenet_amd import qc_models, qc_train
    from graph_odenet_amd.optim import Adam
    hidden, n_graphs = 16, 20
    torch.manual_seed(11)
    m = getattr(qc_models, name)(node_features=13, edge_features=5, target_features=12, hidden_features=hidden,
                                 s2s_processing_steps=3, dropout=0.0, method="rk4", step_size=0.25)
    p = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    step = qc_train.TrainStep(m, Adam(m.parameters(), lr=1e-3), F.mse_loss, mode=mode)
    ode_keys = {"gamma": "ode.odefunc.norm1.weight", "beta": "ode.odefunc.norm1.bias", "W": "ode.odefunc.gc1.weight",
                "b": "ode.odefunc.gc1.bias"}
    ropt = torch.optim.Adam(list(p.values()), lr=1e-3)
    losses, ref_losses = [], []
    for k in range(5):
        x0, Esrc, etgt, val, _, (xf, ef, batch) = batch_of(n_graphs, hidden, seed=20 + k)
        Etgt = dense_etgt(xf.shape[0], etgt, val)
        target = torch.randn(n_graphs, 12, generator=torch.Generator().manual_seed(50 + k))
        losses.append(float(step(xf.to(DEV), ef.to(DEV), Esrc.to(DEV), Etgt.to(DEV), batch.to(DEV), target.to(DEV))))
        if k == 0:
            for key, q in m.ee.named_parameters():
                assert q.grad is not None and float(q.grad.abs().max()) > 0, "no gradient reaches ee." + key
        ref = RefEdgeODEfunc(hidden, Esrc, etgt, val, torch.zeros(1, hidden, hidden), dtype=torch.float32)
        for a, key in ode_keys.items():
            setattr(ref, a, torch.nn.Parameter(p[key].detach().clone()))
        ropt.zero_grad()
        out, A = _ref_model(p, name, ref, xf, ef, Esrc, Etgt, batch, n_graphs, hidden)
        loss = F.mse_loss(out, target)
        loss.backward(retain_graph=True)
        A.backward(ref.A.grad)                       # the block's edge-matrix gradient, on into the encoder
        for a, key in ode_keys.items():
            p[key].grad = getattr(ref, a).grad
        ropt.step()
        ref_losses.append(float(loss.detach()))
    assert all(l == l and abs(l) != float("inf") for l in losses)
    err = max(abs(a - b) for a, b in zip(losses, ref_losses))
    assert err < 5e-5 * max(1.0, max(ref_losses)), (losses, ref_losses)
