"""Fused backprop through rk4 and dopri5 solves over the edge-conditioned ODE function (qc_ode.EdgeOdeField,
csrc/edge_backprop.hip) on the GPU, against autograd through the plain-torch restatement of tests/test_qc_ode_api.py on
the CPU in float32 and float64 (oracle/solver_ref, unchanged).

Bars: noise_floor_check of tests/test_gpu_gcn.py - the error against float64 within slack x the float32 restatement's own
error + 1e-5 x scale - with slack 4, and 20 at h = 16 (slack_of of tests/test_gpu_qc_ode.py).

Launch counts come from the gode_prof_* kinds where the profile brackets the launch.  It brackets the dense launches
(kinds 1 and 3) on their MFMA kernels only: gode_gn_time_gemm_xout_aux_f32 and gode_wgrad_f32 in csrc/gemm.hip dispatch on
fast_cg(), which knows 0, 1, 2 and 4 channels per group, and the narrow / generic kernels they fall through to at h = 96
(three channels per group) are launched without a gode_prof_begin.  There those launches are counted by their calls."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_gcn import noise_floor_check
from test_gpu_large_adjoint import profiled
from test_gpu_qc_ode import NAMES, PNAMES, batch_of, block_run, dense_etgt, product, ref_pair, slack_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KEYS = NAMES + ("x", "y")


def check(got, ref32, ref64, what, slack=4.0):
    """noise_floor_check, the figures printed first."""
    e_ref = (ref32.double() - ref64).abs().max().item()
    e_got = (got.detach().cpu().double() - ref64).abs().max().item()
    print("%-28s err %.3e  float32 restatement err %.3e  scale %.2e" % (what, e_got, e_ref, max(1.0, ref64.abs().max().item())))
    noise_floor_check(got, ref32, ref64, what, slack=slack)


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------
def hub_batch(h, seed=0, n=11, E=30):
    """n = 11 atoms, 30 edges: atom 0 has 20 outgoing edges (more than one round of 16), atoms 9 and 10 have none, atom 10 is
    no edge's target."""
    g = torch.Generator().manual_seed(seed)
    src = torch.cat([torch.zeros(20, dtype=torch.int64), torch.randint(1, 9, (E - 20,), generator=g)])
    tgt = torch.randint(0, n - 1, (E,), generator=g)
    perm = torch.randperm(E, generator=g)
    src, tgt = src[perm], tgt[perm]
    tgt[0] = n - 2                                            # product() sizes the batch by the largest target + 2
    val = torch.rand(E, generator=g) + 0.5
    A = torch.randn(E, h, h, generator=g) / h ** 0.5
    assert (src == 0).sum() == 20 and not (src >= 9).any() and not (tgt == n - 1).any()
    return src, tgt, val, A, g


@pytest.mark.parametrize("h", [7, 16, 64, 96])
def test_stage_kernel_against_float64(h):
    from graph_odenet_amd import ops
    n = 11
    src, tgt, val, A, g = hub_batch(h)
    f, _ = product(h, src, tgt, val, A)
    Ys = [torch.randn(n, h, generator=g) for _ in range(3)]
    Cs = [torch.randn(n, h, generator=g) for _ in range(3)]
    yc, cc, scale, t = (1.0, 0.3, -0.2), (0.5, -1.25, 2.0), 0.7, 0.375
    fwd = f.gode_fields(Ys[0].to(DEV))[0]
    s, es = fwd.s, fwd.s.es
    assert ops.edge_ode_stage_bwd_supported(n, h, s.groups) and fwd.rk4_backprop is not None
    y_terms = [(c, y.to(DEV)) for c, y in zip(yc, Ys)]
    c_terms = [(c, y.to(DEV)) for c, y in zip(cc, Cs)]
    k = torch.empty(n, h, device=DEV)
    fwd.eval(t, [y_terms], [k])
    runs = []
    for _ in range(2):
        o = {key: torch.full((n, h), float("nan"), device=DEV) for key in ("dM", "dS", "ybar", "gr", "br", "S")}
        ops.edge_ode_stage_bwd(es.Ms_inc, es.edge_row, es.edge_val, s.A, c_terms, scale, k, y_terms, t, s.gamma, s.beta, s.W,
                               s.groups, s.eps, o["dM"], o["dS"], o["ybar"], o["gr"], o["br"], S=o["S"])
        runs.append(o)
    for key in runs[0]:
        assert torch.equal(runs[0][key], runs[1][key]), "not deterministic: " + key
    o = runs[0]
    got = {"dM": o["dM"], "dS": o["dS"], "ybar": o["ybar"], "S": o["S"], "dgamma": o["gr"].double().sum(0), "dbeta": o["br"].double().sum(0)}
    want = []
    for ref in ref_pair(f, h, src, tgt, val, A):
        dt = ref.W.dtype
        Y = sum(c * y.to(dt) for c, y in zip(yc, Ys)).requires_grad_(True)
        cot = scale * sum(c * y.to(dt) for c, y in zip(cc, Cs))
        xx = torch.cat([torch.ones(n, 1, dtype=dt) * t, F.group_norm(Y, ref.groups, ref.gamma, ref.beta, ref.eps)], 1)
        S0 = torch.mm(xx, ref.W)
        Sl = S0.detach().requires_grad_(True)
        msg = torch.bmm(ref.A, Sl.index_select(0, ref.Esrc).unsqueeze(-1)).squeeze(-1)
        out = F.relu(torch.zeros(n, h, dtype=dt).index_add_(0, ref.etgt, ref.val.unsqueeze(1) * msg) + ref.b)
        (dS,) = torch.autograd.grad(out, Sl, cot)
        ybar, dg, db = torch.autograd.grad(S0, (Y, ref.gamma, ref.beta), dS)
        want.append({"dM": cot * (out.detach() > 0), "dS": dS, "ybar": ybar, "S": S0.detach(), "dgamma": dg, "dbeta": db})
    for key in got:
        check(got[key], want[0][key], want[1][key], "stage h=%d %s" % (h, key), slack=slack_of(h))


@pytest.mark.parametrize("n,h,q", [(330, 96, 7), (11, 7, 4)])
def test_step_close_against_float64(n, h, q):
    from graph_odenet_amd import _lib, ops
    g = torch.Generator().manual_seed(3)
    npw = _lib.load().gode_wgrad_parts(n)
    wlen = (h + 1) * h
    wp = torch.randn(q, npw, wlen, generator=g)
    dM, gr, br = (torch.randn(q, n, h, generator=g) for _ in range(3))
    ts = [0.1 + 0.17 * i for i in range(q)]
    theta0 = torch.randn(wlen + 3 * h + 5, generator=g)      # non-zero, and a tail the launch must leave alone

    def expected(dt):
        th = theta0.to(dt).clone()
        for i in range(q):
            w = wp[i].to(dt).sum(0)
            w[:h] *= ts[i]
            th[:wlen] += w
            for j, arr in enumerate((dM, gr, br)):
                th[wlen + j * h:wlen + (j + 1) * h] += arr[i].to(dt).sum(0)
        return th
    outs = []
    for _ in range(2):
        th = theta0.to(DEV).clone()
        ops.edge_ode_step_close([(wp[i].to(DEV), dM[i].to(DEV), gr[i].to(DEV), br[i].to(DEV), ts[i]) for i in range(q)], n, h, th)
        outs.append(th)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0][wlen + 3 * h:].cpu(), theta0[wlen + 3 * h:])
    noise_floor_check(outs[0], expected(torch.float32), expected(torch.float64), "step close %d stages" % q)


# ---- whole solves -----------------------------------------------------------------------------------------------------------
def solve_run(f, Ad, x0, R, t, method=None, step_size=None, tol=1e-5, replay=None):
    """odeint with gradients -> (gradients and outputs, (nfe forward, nfe backward), launch kinds, attempt sequences)."""
    from graph_odenet_amd import odeint as OI, solver
    f.zero_grad(set_to_none=True)
    Ad.grad = None
    x = x0.to(DEV).requires_grad_(True)
    f.nfe = 0
    solver.TRACE = []
    solver.REPLAY = [list(seq) for seq in replay] if replay is not None else None
    try:
        with profiled() as kinds:
            out = OI.odeint(f, x, torch.tensor(t, device=DEV), rtol=tol, atol=tol, method=method,
                            options=None if step_size is None else {"step_size": step_size})
            nfe_f, f.nfe = f.nfe, 0
            assert out.grad_fn is not None
            (out * R.to(DEV)).sum().backward()
        trace = solver.TRACE
    finally:
        solver.TRACE = solver.REPLAY = None
    sd = f.state_dict(keep_vars=True)
    g = {k: sd[PNAMES[k]].grad.clone() for k in PNAMES}
    g.update(x=x.grad.clone(), y=out.detach().clone())
    if Ad.grad is not None:
        g["A"] = Ad.grad.clone()
    return g, (nfe_f, f.nfe), [k & 0xff for k in kinds], trace


def plain_solve(f, x0, t, method=None, step_size=None, tol=1e-5):
    from graph_odenet_amd import odeint as OI
    with torch.no_grad():
        out = OI.odeint(f, x0.to(DEV), torch.tensor(t, device=DEV), rtol=tol, atol=tol, method=method,
                        options=None if step_size is None else {"step_size": step_size})
    assert out.grad_fn is None
    return out


def unrolled_rk4(ref, x0, R, t, step):
    """Autograd through the restatement's 3/8-rule steps on the grid odeint takes, loss sum_i <y(t_i), R_i>."""
    from oracle import solver_ref as S
    dt = ref.W.dtype
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
    g = torch.autograd.grad((out * R.to(dt)).sum(), (ref.gamma, ref.beta, ref.W, ref.b, ref.A, x))
    return dict(zip(NAMES + ("x",), g), y=out.detach())


@functools.lru_cache(maxsize=None)
def rk4_case(h):
    """batch_of(20, h, seed=7), t = [0, .5, 1], step 0.25, a loss on every output time: inputs and the two restatements."""
    x0, Esrc, etgt, val, A, _ = batch_of(20, h, seed=7)
    t = [0.0, 0.5, 1.0]
    R = torch.randn((3,) + tuple(x0.shape), generator=torch.Generator().manual_seed(4))
    f, Ad = product(h, Esrc, etgt, val, A)
    want = [unrolled_rk4(ref, x0, R, t, 0.25) for ref in ref_pair(f, h, Esrc, etgt, val, A)]
    return f, Ad, x0, R, t, want


@pytest.mark.parametrize("h", [96, 16])
def test_rk4_against_unrolled_autograd(h):
    f, Ad, x0, R, t, want = rk4_case(h)
    got, nfe, kinds, _ = solve_run(f, Ad, x0, R, t, "rk4", 0.25)
    assert nfe == (16, 0)
    assert kinds.count(9) == 16, "the fused sweep did not run"
    assert torch.equal(got["y"], plain_solve(f, x0, t, "rk4", 0.25)), "forward differs from odeint under no_grad"
    for k in KEYS:
        noise_floor_check(got[k], want[0][k], want[1][k], "rk4 h=%d %s" % (h, k), slack=slack_of(h))


def test_rk4_forward_bit_identical_h64():
    from graph_odenet_amd import odeint as OI
    x0, Esrc, etgt, val, A, _ = batch_of(20, 64, seed=7)
    f, Ad = product(64, Esrc, etgt, val, A)
    t = [0.0, 0.5, 1.0]
    with profiled() as kinds:
        out = OI.odeint(f, x0.to(DEV).requires_grad_(True), torch.tensor(t, device=DEV), method="rk4", options={"step_size": 0.25})
    assert out.grad_fn is not None and [k & 0xff for k in kinds].count(5) == 16
    assert torch.equal(out.detach(), plain_solve(f, x0, t, "rk4", 0.25))


@pytest.mark.parametrize("h", [96, 64])
def test_launch_accounting(h, monkeypatch):
    """The reverse of an rk4 step of 4 stages: 4 stage launches, 4 weight-gradient launches, one closing launch, one
    outer-sum pass and at most one combine; no VJP kernel of the adjoint, no forward kernel.  The profile brackets the dense
    launches (kinds 1 and 3) on their MFMA kernels only, which h = 64 takes and h = 96 (three channels per group) does
    not: there the same launches are counted by their calls, as test_launches_per_evaluation_and_per_vjp counts
    reduce_segments_."""
    from graph_odenet_amd import ops, qc_models, qc_ode
    x0, Esrc, etgt, val, A, (xf, ef, batch) = batch_of(20, h, seed=7)
    f, Ad = product(h, Esrc, etgt, val, A)
    R = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4))
    calls, phase = [], ["fwd"]
    for name in ("lincomb_", "lincomb_multi_", "gn_time_gemm", "wgrad", "edge_ode_vjp", "gn_time_gemm_bwd", "reduce_segments_"):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _n=name, **k: (calls.append((_n, phase[0])), _o(*a, **k))[1])
    blk = qc_ode.EdgeODEBlock(f, method="rk4", step_size=0.25, adjoint=False)
    x = x0.to(DEV).requires_grad_(True)
    with profiled() as kinds:
        y = blk(x, f.Esrc, f.Etgt, Ad)
        phase[0] = "bwd"
        (y * R.to(DEV)).sum().backward()
    fam = [k & 0xff for k in kinds]
    assert fam.count(5) == 16 and fam.count(9) == 16 and fam.count(10) == 4 and fam.count(7) == 4, sorted(set(fam))
    assert 2 not in fam and 6 not in fam and 8 not in fam
    assert calls.count(("gn_time_gemm", "fwd")) == 16 and calls.count(("wgrad", "bwd")) == 16
    assert not [c for c in calls if c[0] in ("edge_ode_vjp", "gn_time_gemm_bwd", "reduce_segments_")]
    assert ("gn_time_gemm", "bwd") not in calls and ("wgrad", "fwd") not in calls
    if h == 64:
        assert fam.count(1) == 16 and fam.count(3) == 16
    assert sum(1 for c in calls if c[0].startswith("lincomb") and c[1] == "bwd") <= 4
    if h != 96:
        return
    torch.manual_seed(11)
    m = qc_models.EdgeODE1_K_Sum(node_features=13, edge_features=5, target_features=12, hidden_features=96, dropout=0.0,
                                 method="rk4", step_size=0.25, adjoint=False).to(DEV).train()
    Etgt = dense_etgt(xf.shape[0], etgt, val)
    with profiled() as kinds:
        m(xf.to(DEV), ef.to(DEV), Esrc.to(DEV), Etgt.to(DEV), batch.to(DEV)).sum().backward()
    fam = [k & 0xff for k in kinds]
    assert fam.count(9) == 16 and fam.count(10) == 4 and 6 not in fam
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in m.ee.parameters())


def test_rk4_rerun_mode_bit_identical(monkeypatch):
    from graph_odenet_amd import odeint as OI
    f, Ad, x0, R, t, _ = rk4_case(96)
    got, _, kinds, _ = solve_run(f, Ad, x0, R, t, "rk4", 0.25)
    monkeypatch.setattr(OI, "BACKPROP_SAVE_MAX_BYTES", 0)
    rec, nfe, kinds_r, _ = solve_run(f, Ad, x0, R, t, "rk4", 0.25)
    assert kinds_r.count(9) == 16 and kinds_r.count(5) == 32 and nfe == (16, 0)      # every step run twice, counted once
    for k in KEYS:
        assert torch.equal(rec[k], got[k]), k


def test_no_edge_gradient():
    """edge_data without requires_grad: the four parameter gradients (bit for bit those of the run with it), no outer sum."""
    f, Ad, x0, R, t, _ = rk4_case(96)
    full, _, _, _ = solve_run(f, Ad, x0, R, t, "rk4", 0.25)
    Esrc, Etgt = f.Esrc, f.Etgt
    f.set_edges(Esrc, Etgt, Ad.detach())
    try:
        got, _, kinds, _ = solve_run(f, Ad, x0, R, t, "rk4", 0.25)
    finally:
        f.set_edges(Esrc, Etgt, Ad)
    assert "A" not in got and kinds.count(9) == 16 and kinds.count(10) == 4 and 7 not in kinds and 8 not in kinds
    for k in tuple(PNAMES) + ("x", "y"):
        assert torch.equal(got[k], full[k]), k


# ---- dopri5 ---------------------------------------------------------------------------------------------------------------
def oracle_dopri5(ref, x0, R, tol, trace):
    from oracle import solver_ref as S
    dt = ref.W.dtype
    ref.zero_grad(set_to_none=True)
    x = x0.detach().clone().to(dt).requires_grad_(True)
    S.REPLAY = [list(seq) for seq in trace]
    try:
        out = S.odeint(ref, x, torch.tensor([0.0, 1.0], dtype=dt), rtol=tol, atol=tol, method="dopri5")
        assert S.REPLAY == []
    finally:
        S.REPLAY = None
    (out * R.to(dt)).sum().backward()
    g = {k: getattr(ref, k).grad.clone() for k in NAMES}
    g.update(x=x.grad.clone(), y=out.detach().clone())
    return g


@functools.lru_cache(maxsize=None)
def dopri5_case(tol):
    """batch_of(20, 96, seed=7) under dopri5 at rtol = atol = tol: the fused run, and autograd through the oracle solver on
    the product's own attempt sequence in float32 and float64."""
    h = 96
    x0, Esrc, etgt, val, A, _ = batch_of(20, h, seed=7)
    R = torch.zeros((2,) + tuple(x0.shape))
    R[1] = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4))
    f, Ad = product(h, Esrc, etgt, val, A)
    run = solve_run(f, Ad, x0, R, [0.0, 1.0], tol=tol)
    want = [oracle_dopri5(ref, x0, R, tol, run[3]) for ref in ref_pair(f, h, Esrc, etgt, val, A)]
    return f, Ad, x0, R, run, want


def check_dopri5(tol):
    f, Ad, x0, R, (got, nfe, kinds, trace), want = dopri5_case(tol)
    (seq,) = trace
    acc = [a[0] for a in seq if a[1]]
    print("attempts %d, accepted %d, last abscissa %.3f" % (len(seq), len(acc), (1.0 - sum(acc[:-1])) / acc[-1]))
    assert len(acc) >= 2
    assert (1.0 - sum(acc[:-1])) / acc[-1] < 1.0, "the last step must overshoot t = 1 and be interpolated"
    assert 1 <= kinds.count(9) <= 6 * len(acc) + 1 and 2 not in kinds and 6 not in kinds
    assert kinds.count(10) == len(acc) and kinds.count(7) == len(acc)
    assert nfe == (2 + 6 * len(seq), 0)
    assert torch.equal(got["y"], plain_solve(f, x0, [0.0, 1.0], tol=tol)), "forward differs from odeint under no_grad"
    for k in KEYS:
        noise_floor_check(got[k], want[0][k], want[1][k], "dopri5 %g %s" % (tol, k))
    return seq


def test_dopri5_against_the_oracle_on_the_products_own_steps():
    check_dopri5(1e-3)


def test_dopri5_rejected_attempts_contribute_nothing():
    seq = check_dopri5(1e-5)
    assert sum(1 for a in seq if not a[1]) >= 1, seq


def test_dopri5_generic_path_at_the_same_noise_floor():
    """BACKPROP_FUSED = False: the field offers no sweep and every accepted step is re-run as torch ops under autograd."""
    from graph_odenet_amd import qc_ode
    f, Ad, x0, R, (_, _, _, trace), want = dopri5_case(1e-3)
    qc_ode.EdgeOdeField.BACKPROP_FUSED = False
    try:
        assert f.gode_fields(x0.to(DEV))[0].dopri5_step_backprop is None
        got, _, kinds, trace_g = solve_run(f, Ad, x0, R, [0.0, 1.0], tol=1e-3, replay=trace)
    finally:
        qc_ode.EdgeOdeField.BACKPROP_FUSED = True
    assert 9 not in kinds and 10 not in kinds
    assert [[a[:2] for a in seq] for seq in trace_g] == [[a[:2] for a in seq] for seq in trace]
    for k in KEYS:
        noise_floor_check(got[k], want[0][k], want[1][k], "dopri5 generic " + k)


def test_large_batch_keeps_the_generic_path(monkeypatch):
    """4 438 edges (spec.large): no sweep on the instance, gradients from the generic path at the unrolled restatement's
    noise floor.  No launch of this route at h = 96 is one the profile brackets (the module docstring says why; an empty
    profile makes profiled() itself fail), so the stage kernel (kind 9) is shown absent by its calls."""
    from graph_odenet_amd import ops
    h = 96
    x0, Esrc, etgt, val, A, _ = batch_of(120, h, seed=7)
    assert Esrc.numel() >= ops.EDGE_ODE_FUSED_MAX_EDGES
    R = torch.randn(x0.shape, generator=torch.Generator().manual_seed(4))
    f, Ad = product(h, Esrc, etgt, val, A)
    fwd = f.gode_fields(x0.to(DEV))[0]
    assert fwd.rk4_forward_save is None and fwd.dopri5_step_backprop is None and fwd.packed_grads is None
    Rs = torch.stack([torch.zeros_like(R), R])
    want = [unrolled_rk4(ref, x0, Rs, [0.0, 1.0], 0.5) for ref in ref_pair(f, h, Esrc, etgt, val, A)]
    calls = []
    for name in ("edge_ode_stage_bwd", "edge_ode_step_close"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    got, _ = block_run(f, Ad, x0, R, "rk4", 0.5, adjoint=False)
    assert not calls
    for k in KEYS:
        w32, w64 = (w[k][1] if k == "y" else w[k] for w in want)
        noise_floor_check(got[k], w32, w64, "large generic " + k)
