"""bosh3 and adaptive_heun on the GAT and edge-conditioned fields through the one-call step and the fused sweeps
(csrc/gat_small.hip: gode_gat_small_finish_multi_f32; csrc/gat_driver.hip: gode_gat_ode_adaptive_step_*; gat_ode.py,
qc_ode.py), on the GPU.  Graphs: those of test_gpu_adaptive_methods.test_gat_bosh3 - 300 nodes, random edges with a self
loop per node.  Bits are compared with torch.equal; everything else by noise_floor_check against the float32 and float64
restatements of tests/adaptive_methods_ref.py replaying the product's own attempt sequences."""
import functools

import pytest
import torch

import adaptive_methods_ref as A
import fixed_methods_ref as R
from test_gpu_adaptive_methods import accepted, check_all, end_weights, product_run, refs_for

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEW = ["bosh3", "adaptive_heun"]
N = 300
WIDTHS = [(16, 1), (64, 8)]                          # one head x 16, 8 heads x 8


@pytest.fixture(autouse=True)
def adaptive_native_on():
    """The GAT fields' one-call step and sweep under bosh3 / adaptive_heun are an opt-in (gat_ode.GatOdeField.ADAPTIVE_NATIVE):
    every test here runs with it on; test_members_absent_with_the_switch_off has the default."""
    from graph_odenet_amd import gat_ode
    old = gat_ode.GatOdeField.ADAPTIVE_NATIVE
    gat_ode.GatOdeField.ADAPTIVE_NATIVE = True
    yield
    gat_ode.GatOdeField.ADAPTIVE_NATIVE = old


# ---- 1. the closing launch of an adjoint step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [5, 300, 4100])
@pytest.mark.parametrize("d,H", [(16, 1), (32, 2), (64, 8)])
def test_finish_multi_is_the_single_launch_bit_for_bit(d, H, n_rows):
    """n_stages = 1, 3, 6, 7 over random partial slots against that many gode_gat_small_finish_f32 calls: every ktheta and kat
    torch.equal, the 8 guard floats after each output untouched.  gode_gat_small_parts never exceeds 512 (d = 16) / 256
    (d = 32, 64), so the 16 x 32 load loop has one round everywhere; n_rows = 4 100 is at the cap of every width, the largest
    count it gives."""
    from graph_odenet_amd import _lib, ops
    lib = _lib.load()
    n_part = lib.gode_gat_small_parts(n_rows, d)
    if n_rows == 4100:
        assert n_part == (512 if d == 16 else 256) and lib.gode_gat_small_parts(65536, d) == n_part
    slot = n_part * lib.gode_gat_small_part_len(d, H)
    nth = lib.gode_gat_ode_theta_len_heads(d, H)
    g = torch.Generator().manual_seed(1000 * d + n_rows)
    parts = torch.randn(7 * slot, generator=g).to(DEV)
    ts_all = [0.1 + 0.17 * s for s in range(7)]
    ref = []
    for s in range(7):
        kth, kat = torch.empty(nth, device=DEV), torch.empty(1, device=DEV)
        ops.gat_small_finish(parts[s * slot:(s + 1) * slot], n_rows, d, H, ts_all[s], kth, kat)
        ref.append((kth, kat))
    for q in (1, 3, 6, 7):
        kth = [torch.full((nth + 8,), float("nan"), device=DEV) for _ in range(q)]
        kat = [torch.full((9,), float("nan"), device=DEV) for _ in range(q)]
        ops.gat_small_finish_multi(parts, n_rows, d, H, ts_all[:q], [x[:nth] for x in kth], [x[:1] for x in kat])
        torch.cuda.synchronize()
        for s in range(q):
            assert torch.equal(kth[s][:nth], ref[s][0]), (q, s, "ktheta")
            assert torch.equal(kat[s][:1], ref[s][1]) and bool(torch.isfinite(kat[s][0])), (q, s, "kat")
            assert bool(torch.isnan(kth[s][nth:]).all()) and bool(torch.isnan(kat[s][1:]).all()), (q, s, "guards")


# ---- the GAT functions ----------------------------------------------------------------------------------------------------------
def gat_func(d, H, E=1400, seed=5, act=None):
    """gat_models.ODEfunc (one head) / gat_heads.ODEfunc (H heads) on N nodes and E random edges with self loops, GroupNorm's
    affine pair away from (1, 0) -> (f, src, tgt)."""
    from graph_odenet_amd import gat_heads, gat_models
    src, tgt = R.random_edges(N, E, 17)
    torch.manual_seed(seed)
    kw = {} if act is None else {"act": act}
    f = gat_models.ODEfunc(d, **kw) if H == 1 else gat_heads.ODEfunc(d, H, **kw)
    with torch.no_grad():
        f.norm1.weight.add_(0.3 * torch.randn(d))
        f.norm1.bias.add_(0.3 * torch.randn(d))
    f = f.to(DEV)
    f.set_adj(src.to(DEV), tgt.to(DEV), R.mtgt(N, tgt).to(DEV))
    return f, src, tgt


def start_state(d, seed=9):
    """0.5 randn; at d = 64 (two channels per GroupNorm group, whose backward scales with 1 / |x_a - x_b|) the two channels
    of every pair start 6 apart, as tests/test_gpu_gat_backprop.py: x0_of explains."""
    g = torch.Generator().manual_seed(seed)
    x = 0.5 * torch.randn(N, d, generator=g)
    if d == 64:
        s = 3.0 * (2.0 * torch.randint(0, 2, (N, d // 2), generator=g) - 1.0)
        x[:, 0::2] += s
        x[:, 1::2] -= s
    return x


def pnames(f):
    return [k for k, _ in f.named_parameters()]


# ---- 2. the new drivers on GODE_RKA_DOPRI5 are the dopri5 drivers ----------------------------------------------------------------
# (d, H, E, small_fused, act); raw: whether the H-head case takes the raw-logit route.  The kernels see the H-fold graph, so
# 8 heads on 1 400 edges are 11 200 edges there - past 8 192 like the 9 000-edge case; the 900-edge case (7 200) is the one
# on shifted logits.
ROUTES = {
    "one-head-16": (16, 1, 1400, 1, None),
    "one-head-64": (64, 1, 1400, 1, None),
    "heads-8x8-E1400": (64, 8, 1400, 1, None),
    "heads-8x8-E9000": (64, 8, 9000, 1, None),
    "heads-8x8-E900-shifted": (64, 8, 900, 1, None),
    "one-head-16-separate-launches": (16, 1, 1400, 0, None),
    "one-head-16-elu": (16, 1, 1400, 1, "elu"),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_new_drivers_on_dopri5_equal_the_dopri5_drivers(route, monkeypatch):
    """GODE_RKA_DOPRI5 through gode_gat_ode_adaptive_step_forward / _adjoint / _backprop against gode_gat_ode_dopri5_step_* on
    the same inputs (the fields' members): every output array and every sum under torch.equal - the adjoint with `parts`
    (one gode_gat_small_finish_multi_f32) and without, the backprop opening an interval and inside one with a kbar_last.
    With small_fused 0 both backprops refuse (GODE_E_UNSUPPORTED)."""
    import torch.nn.functional as F
    from graph_odenet_amd import _lib, solver
    lib = _lib.load()
    d, H, E, small_fused, act = ROUTES[route]
    f, _, _ = gat_func(d, H, E, act=F.elu if act == "elu" else None)
    g = torch.Generator().manual_seed(5)
    x0 = start_state(d).to(DEV)
    t, h, tol = 0.25, 0.3, 1e-3
    old = lib.gode_get_option(b"small_fused")
    lib.gode_set_option(b"small_fused", small_fused)
    try:
        fwd, mk_adj, _ = f.gode_fields(x0)
        fwd.prepare()
        assert fwd.small() == bool(small_fused)
        if H > 1:
            assert fwd.raw_logits() == (E * H > 8192), "route"
        if act is not None:
            assert fwd._kernel_act()[0] is not None
        # forward
        res = {}
        for which in ("old", "new"):
            kk = [[torch.zeros(N, d, device=DEV)] for _ in range(7)]
            fwd.eval(t, [[(1.0, x0)]], kk[0])
            y1 = [torch.empty(N, d, device=DEV)]
            step = fwd.dopri5_step_native if which == "old" else functools.partial(fwd.adaptive_step_native, "dopri5")
            sums = step([x0], kk, y1, t, h, tol, tol)
            torch.cuda.synchronize()
            res[which] = [y1[0]] + [k[0] for k in kk] + [sums]
        assert res["old"][1].abs().max().item() > 1e-2, "k must not be tiny"
        for i, (a, b) in enumerate(zip(res["old"], res["new"])):
            assert torch.equal(a, b), ("forward", i)
        ks = res["old"][1:8]
        # backprop over that step, opening an interval (first) and inside one
        gbar = torch.randn(N, d, generator=g).to(DEV)
        kb7 = torch.randn(N, d, generator=g).to(DEV) * 0.1
        wk = [h * b for b in A.TABLEAUS["dopri5"][2]]
        wk[6] = 0.01 * h
        for first, kbar in ((True, None), (False, kb7)):
            if not small_fused:
                assert fwd.dopri5_step_backprop is None and fwd.adaptive_step_backprop is None
                work = fwd._dopri5_backprop_work(gbar)
                theta = fwd._packed_grads(DEV)
                with pytest.raises(Exception, match="gode_gat_ode_dopri5_step_backprop"):
                    fwd._dopri5_step_backprop(x0, ks, gbar, kbar, 0.9, wk, t, h, first, work, 0, theta)
                with pytest.raises(Exception, match="gode_gat_ode_adaptive_step_backprop"):
                    fwd._adaptive_step_backprop("dopri5", x0, ks, gbar, kbar, 0.9, wk, t, h, first, work, 0, theta)
                continue
            out = {}
            for which in ("old", "new"):
                theta = fwd.packed_grads(DEV)
                if which == "old":
                    work = fwd.dopri5_backprop_work(gbar)
                    yb, kb1 = fwd.dopri5_step_backprop(x0, ks, gbar, kbar, 0.9, wk, t, h, first, work, 0, theta)
                else:
                    work = fwd.adaptive_backprop_work("dopri5", gbar)
                    yb, kb1 = fwd.adaptive_step_backprop("dopri5", x0, ks, gbar, kbar, 0.9, wk, t, h, first, work, 0, theta)
                torch.cuda.synchronize()
                out[which] = [yb.clone(), theta.clone()] + ([] if kb1 is None else [kb1.clone()])
            assert out["old"][1].abs().max().item() > 0
            for i, (a, b) in enumerate(zip(out["old"], out["new"])):
                assert torch.equal(a, b), ("backprop", first, i)
        # adjoint: the dopri5 driver, the new one with `parts` and the new one with parts = NULL
        adj_f = mk_adj()
        adj_f.prepare()
        res = {}
        for which in ("old", "parts", "null"):
            y = adj_f.new_state(x0)
            y[1].copy_(gbar)
            kk = solver._alloc_like(y, 7)
            for k in kk[1:]:
                for c in k:
                    c.fill_(float("nan"))
            adj_f.eval(t, [[(1.0, c)] for c in y], kk[0])
            (y1,) = solver._alloc_like(y, 1)
            if which == "null":
                monkeypatch.setattr(adj_f, "_adjoint_parts", lambda S: None)
            elif which == "parts":
                assert (adj_f._adjoint_parts(7) is not None) == bool(small_fused)
            step = adj_f.dopri5_step_native if which == "old" else functools.partial(adj_f.adaptive_step_native, "dopri5")
            sums = step(y, kk, y1, t, -h, tol, tol)
            torch.cuda.synchronize()
            res[which] = list(y1) + [c for k in kk for c in k] + [sums]
        assert res["old"][-1].numel() == 4
        for which in ("parts", "null"):
            for i, (a, b) in enumerate(zip(res["old"], res[which])):
                assert torch.equal(a, b), ("adjoint", which, i)
    finally:
        lib.gode_set_option(b"small_fused", old)


# ---- 3. the one-call step against the per-stage driver --------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", WIDTHS)
@pytest.mark.parametrize("method", NEW)
def test_native_step_against_per_stage_driver(method, d, H, monkeypatch):
    """odeint_adjoint on the product's own attempt sequences (replayed), solver.DOPRI5_NATIVE on and off: the C and the Python
    driver issue the same launches, the closing launch of the stages and the close of the step are bit-exact, so y(1),
    dL/dx0 and every parameter gradient are torch.equal."""
    from graph_odenet_amd import solver
    f, _, _ = gat_func(d, H)
    x0, Rw = start_state(d), end_weights((N, d), 10)
    free = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, True)
    trace = free[4]
    assert len(trace) == 2 and len(accepted(trace[0])) >= 2
    native = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, True, replay=trace)
    assert native[3] == free[3] and torch.equal(native[0], free[0]) and torch.equal(native[1], free[1])
    monkeypatch.setattr(solver, "DOPRI5_NATIVE", False)
    stage = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, True, replay=trace)
    assert stage[3] == native[3]
    assert [(a[0], a[1]) for s in stage[4] for a in s] == [(a[0], a[1]) for s in native[4] for a in s]
    assert torch.equal(stage[0], native[0]), "y(1)"
    assert torch.equal(stage[1], native[1]), "dL/dx0"
    for k, a, b in zip(pnames(f), stage[2], native[2]):
        assert torch.equal(a, b), k
    assert [a[2] for s in stage[4] for a in s] == [a[2] for s in native[4] for a in s], "error ratios"


# ---- 4. against float64 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float64_case(method, d, H, adjoint):
    """The product's run at rtol = atol = 1e-3 with its generic path made to raise, and the two restatements on its attempt
    sequences."""
    from graph_odenet_amd import odeint as OI
    f, src, tgt = gat_func(d, H)
    x0, Rw = start_state(d), end_weights((N, d), 10)

    def boom(*a, **k):
        raise AssertionError("the generic backprop ran")
    saved = OI._dopri5_step_torch
    OI._dopri5_step_torch = boom
    try:
        got = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, adjoint)
    finally:
        OI._dopri5_step_torch = saved
    refs = refs_for(lambda dt: R.GatRef(f, N, src, tgt, dt), x0, [0.0, 1.0], Rw, method, 1e-3, adjoint, got[4])
    return f, got, refs


@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("d,H", WIDTHS)
@pytest.mark.parametrize("method", NEW)
def test_against_float64(method, d, H, adjoint):
    """y(1), dL/dx0 and every parameter gradient through odeint_adjoint and through odeint (the fused sweep: the generic
    path raises) at the restatement's noise floor; nfe as the restatement counts it."""
    f, got, refs = float64_case(method, d, H, adjoint)
    seq = got[4][0]
    print("%s d=%d H=%d attempts %s" % (method, d, H, [(round(a[0], 4), a[1]) for a in seq]))
    assert len(accepted(seq)) >= 2 and len(got[4]) == (2 if adjoint else 1)
    S = A.STAGES[method]
    assert got[3][0] == 2 + (S - 1) * len(seq)
    if not adjoint:
        assert got[3][1] == 0
    check_all(got, refs, "gat %s d=%d H=%d %s" % (method, d, H, "adjoint" if adjoint else "backprop"), pnames(f))


# ---- 5. the members --------------------------------------------------------------------------------------------------------------
MEMBERS = ("adaptive_step_native", "adaptive_step_backprop", "adaptive_backprop_work")


@pytest.mark.parametrize("d,H", WIDTHS)
def test_members_on_the_launch_bound_fields(d, H):
    from graph_odenet_amd import _lib
    lib = _lib.load()
    f, _, _ = gat_func(d, H)
    x0 = start_state(d).to(DEV)
    fwd, mk_adj, _ = f.gode_fields(x0)
    assert fwd.small() and not fwd.s.pad_logits
    for name in MEMBERS:
        assert getattr(fwd, name) is not None, name
    adj = mk_adj()
    assert adj.adaptive_step_native is not None and adj.adaptive_step_backprop is None
    lib.gode_set_option(b"small_fused", 0)
    try:
        off = f.gode_fields(x0)[0]
        assert off.adaptive_step_native is not None                 # the step has the separate launches
        assert off.adaptive_step_backprop is None and off.adaptive_backprop_work is None
        assert off.dopri5_step_backprop is None
    finally:
        lib.gode_set_option(b"small_fused", 1)


def test_members_absent_with_the_switch_off():
    """ADAPTIVE_NATIVE off (the default): no adaptive member on either field, the dopri5 members as before."""
    from graph_odenet_amd import gat_ode
    gat_ode.GatOdeField.ADAPTIVE_NATIVE = False          # the fixture restores it
    f, _, _ = gat_func(16, 1)
    fwd, mk_adj, _ = f.gode_fields(start_state(16).to(DEV))
    for name in MEMBERS:
        assert getattr(fwd, name) is None, name
    assert fwd.dopri5_step_native is not None and fwd.dopri5_step_backprop is not None
    adj = mk_adj()
    assert adj.adaptive_step_native is None and adj.dopri5_step_native is not None


def test_no_members_under_padded_logit_columns():
    """8 heads on 5 000 nodes: the logit columns ride a padded block (pad_logits), where dopri5_step_native is None - and so
    are the three adaptive members, on the forward and the adjoint field."""
    from graph_odenet_amd import gat_heads
    n, E, d, H = 5000, 24000, 32, 8
    g = torch.Generator().manual_seed(12)
    src, tgt = torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)
    torch.manual_seed(8)
    f = gat_heads.ODEfunc(d, H).to(DEV)
    f.set_adj(src.to(DEV), tgt.to(DEV), R.mtgt(n, tgt).to(DEV))
    fwd, mk_adj, _ = f.gode_fields(torch.zeros(n, d, device=DEV))
    assert fwd.s.pad_logits and fwd.dopri5_step_native is None
    for name in MEMBERS:
        assert getattr(fwd, name) is None, name
    adj = mk_adj()
    assert adj.dopri5_step_native is None and adj.adaptive_step_native is None


# ---- 6. recompute mode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H", WIDTHS)
@pytest.mark.parametrize("method", NEW)
def test_recompute_mode_bit_identical(method, d, H, monkeypatch):
    """BACKPROP_SAVE_MAX_BYTES = 0 (below one step's record): every accepted step keeps y_n and k_1 and is re-run by one
    native step call before its sweep - the gradients of the full-record run bit for bit."""
    from graph_odenet_amd import odeint as OI
    f, _, _ = gat_func(d, H)
    x0, Rw = start_state(d), end_weights((N, d), 10)
    full = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, False)
    assert len(accepted(full[4][0])) >= 2
    monkeypatch.setattr(OI, "BACKPROP_SAVE_MAX_BYTES", 0)
    rec = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, False)
    assert rec[4] == full[4] and torch.equal(rec[0], full[0]) and torch.equal(rec[1], full[1])
    for k, a, b in zip(pnames(f), rec[2], full[2]):
        assert torch.equal(a, b), k


# ---- 7. three output times --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", NEW)
def test_three_output_times_and_nfe(method):
    """t = [0, 0.4, 1] with a cotangent on every output, one head x 16: nfe = 2 + (S - 1) attempts per interval (the first
    evaluation and the initial-step probe, then S - 1 per attempt: FSAL) through both gradient paths, three outputs at the
    restatement's noise floor."""
    d, H = 16, 1
    f, src, tgt = gat_func(d, H)
    x0 = start_state(d)
    t = [0.0, 0.4, 1.0]
    Rw = torch.randn((3, N, d), generator=torch.Generator().manual_seed(8))
    S = A.STAGES[method]
    for adjoint in (False, True):
        got = product_run(f, x0, t, Rw, method, 1e-3, adjoint)
        assert got[0].shape[0] == 3 and torch.equal(got[0][0].cpu(), x0)
        trace = got[4]
        assert len(trace) == (4 if adjoint else 2)
        assert got[3][0] == sum(2 + (S - 1) * len(s) for s in trace[:2])
        refs = refs_for(lambda dt: R.GatRef(f, N, src, tgt, dt), x0, t, Rw, method, 1e-3, adjoint, trace)
        check_all(got, refs, "gat 3 times %s %s" % (method, "adjoint" if adjoint else "backprop"), pnames(f))


# ---- 8. the edge-conditioned block ------------------------------------------------------------------------------------------------
EDGE_KEYS = ("gamma", "beta", "W", "b", "A")


@pytest.mark.parametrize("edge_grad", [True, False])
@pytest.mark.parametrize("method", NEW)
def test_edge_block_fused_sweep(method, edge_grad, monkeypatch):
    """EdgeODEBlock(method, adjoint=False) on the 20-molecule batch of test_edge_block_bosh3, h = 16, with and without a
    gradient for edge_data: the field offers the sweep, the generic path raises, and y(1), dL/dx0, the four parameter
    gradients and dL/d(edge_data) sit at the noise floor of RefEdgeODEfunc on the product's attempt sequence."""
    from graph_odenet_amd import odeint as OI, qc_ode, solver
    from test_gpu_qc_ode import PNAMES, batch_of, product
    from test_qc_ode_api import RefEdgeODEfunc
    h = 16
    x0, Esrc, etgt, val, Am, _ = batch_of(20, h, seed=7)
    f, Ad = product(h, Esrc, etgt, val, Am)
    if not edge_grad:
        Ad = Ad.detach()
        f.set_edges(f.Esrc, f.Etgt, Ad)
    fwd = f.gode_fields(x0.to(DEV))[0]
    assert fwd.adaptive_step_backprop is not None and fwd.adaptive_backprop_work is not None and fwd.want_A == edge_grad
    assert fwd.adaptive_step_native is None

    def boom(*a, **k):
        raise AssertionError("the generic backprop ran")
    monkeypatch.setattr(OI, "_dopri5_step_torch", boom)
    Rw = end_weights(x0.shape, 4)
    blk = qc_ode.EdgeODEBlock(f, tol=1e-3, method=method, step_size=None, adjoint=False)
    f.zero_grad(set_to_none=True)
    x = x0.to(DEV).requires_grad_(True)
    solver.TRACE = []
    try:
        f.nfe = 0
        y = blk(x, f.Esrc, f.Etgt, Ad)
        nfe = f.nfe
        (y * Rw[1].to(DEV)).sum().backward()
        torch.cuda.synchronize()
        trace = solver.TRACE
    finally:
        solver.TRACE = None
    assert len(trace) == 1 and len(accepted(trace[0])) >= 2
    assert nfe == 2 + (A.STAGES[method] - 1) * len(trace[0])
    sd = f.state_dict(keep_vars=True)
    got = {k: sd[PNAMES[k]].grad.clone() for k in PNAMES}
    got.update(x=x.grad.clone(), y=y.detach().clone())
    keys = EDGE_KEYS if edge_grad else EDGE_KEYS[:4]
    if edge_grad:
        got["A"] = Ad.grad.clone()
    else:
        assert Ad.grad is None
    pair = {dt: RefEdgeODEfunc(h, Esrc, etgt, val, Am, dtype=dt).load(f) for dt in (torch.float32, torch.float64)}
    (o32, gx32, gp32), (o64, gx64, gp64) = refs_for(lambda dt: pair[dt], x0, [0.0, 1.0], Rw, method, 1e-3, False, trace,
                                                    params_of=lambda r: [getattr(r, k) for k in keys])
    what = "edge %s sweep%s" % (method, "" if edge_grad else " (no edge gradient)")
    R.noise_floor_check(got["y"], o32[1], o64[1], what + " y(1)")
    R.noise_floor_check(got["x"], gx32, gx64, what + " dL/dx0")
    for i, k in enumerate(keys):
        R.noise_floor_check(got[k], gp32[i], gp64[i], what + " dL/d" + k)


# ---- 9. training -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adjoint", [True, False])
def test_gat_ode_block_trains_under_bosh3(golden, adjoint):
    """A linear readout over ODEBlock(gat_models.ODEfunc(16), method='bosh3') on the Citeseer edge list (3 327 nodes, the
    golden fixture): five Adam steps through the one-call adjoint step (adjoint) and the fused sweep (adjoint=False, the
    generic path made to raise); the loss stays finite and decreases, every gradient is finite."""
    import numpy as np
    from graph_odenet_amd import gat_models, odeint as OI
    from graph_odenet_amd.models import ODEBlock
    ge = golden("citeseer_gat_edges.npz")
    n, d = int(ge["n"]), 16
    T = lambda a: torch.from_numpy(np.asarray(a))      # noqa: E731
    src, tgt = T(ge["src"]).long(), T(ge["tgt"]).long()
    assert n == 3327
    args = (src.to(DEV), tgt.to(DEV), R.mtgt(n, tgt).to(DEV))
    torch.manual_seed(5)
    f = gat_models.ODEfunc(d)
    with torch.no_grad():
        f.norm1.weight.add_(0.3 * torch.randn(d))
        f.norm1.bias.add_(0.3 * torch.randn(d))
    blk = ODEBlock(f, method="bosh3", tol=1e-3, adjoint=adjoint).to(DEV)
    torch.manual_seed(2)
    head = torch.nn.Linear(d, 6).to(DEV)
    g = torch.Generator().manual_seed(3)
    x0 = (0.5 * torch.randn(n, d, generator=g)).to(DEV)
    labels = torch.randint(0, 6, (n,), generator=g).to(DEV)
    blk.odefunc.set_adj(*args)
    fwd = blk.odefunc.gode_fields(x0)[0]
    assert fwd.adaptive_step_native is not None and fwd.adaptive_step_backprop is not None

    def boom(*a, **k):
        raise AssertionError("the generic backprop ran")
    saved = OI._dopri5_step_torch
    OI._dopri5_step_torch = boom
    try:
        opt = torch.optim.Adam(list(blk.parameters()) + list(head.parameters()), lr=0.02)
        losses = []
        for _ in range(5):
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(head(blk(x0, *args)), labels)
            loss.backward()
            opt.step()
            losses.append(loss.item())
    finally:
        OI._dopri5_step_torch = saved
    print("losses", losses)
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in blk.parameters())
    assert blk.nfe > 0
