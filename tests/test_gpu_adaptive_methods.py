"""Adaptive bosh3 and adaptive_heun solves on the GPU: the fused step close (csrc/rk.hip) against the launches it replaces,
the tableau-driven step drivers against the dopri5 ones bit for bit, and odeint / odeint_adjoint under the two methods - the
GCN field on its routes, a generic func, the GAT and the edge-conditioned ODE functions - against the float64 restatement of
tests/adaptive_methods_ref.py replaying the product's own attempt sequences (solver.TRACE), on the CPU.

Yardstick: noise_floor_check (tests/test_gpu_gcn.py, copied into fixed_methods_ref) at its slack 4 and floor 1e-5."""
import functools

import numpy as np
import pytest
import torch

import adaptive_methods_ref as A
import fixed_methods_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEW = ["bosh3", "adaptive_heun"]


# ---- 1. the fused close --------------------------------------------------------------------------------------------------------
def _close_case(n, nterms, seed, offset_term=None):
    """Terms y0, k_1.. of length n (one coefficient in the middle zero, also in the error weights), optionally one term
    starting one float past a 16-byte boundary."""
    g = torch.Generator().manual_seed(seed)
    terms = []
    for j in range(nterms):
        buf = torch.randn(n + 4, generator=g).to(DEV)
        terms.append(buf[1:n + 1] if j == offset_term else buf[:n])
    coef = [1.0] + [float(v) for v in (torch.rand(nterms - 1, generator=g) - 0.5)]
    ecoef = [0.0] + [float(v) for v in (torch.rand(nterms - 1, generator=g) - 0.5) * 1e-2]
    if nterms > 2:
        coef[nterms // 2] = 0.0
        ecoef[zero_err_term(nterms)] = 0.0
    return terms, coef, ecoef


def zero_err_term(nterms):
    """The term of a _close_case (nterms > 2) whose error weight is zero while its solution weight is not."""
    return 1 + (nterms // 2) % (nterms - 1)


def _separate(terms, coef, ecoef, rtol, atol):
    """The launches the fused close replaces: gode_lincomb_f32, then gode_rk_errnorm_f32 on its y1 (zero coefficients dropped)."""
    from graph_odenet_amd import ops
    y1 = torch.empty_like(terms[0].contiguous())
    ops.lincomb_(y1, [(c, t) for c, t in zip(coef, terms) if c != 0.0])
    s = ops.rk_error_sumsq(terms[0], y1, [(c, t) for c, t in zip(ecoef, terms) if c != 0.0], rtol, atol)
    return y1, s


def _float64(terms, coef, ecoef, rtol, atol):
    f32 = lambda v: float(np.float32(v))      # noqa: E731
    t64 = [t.double().cpu() for t in terms]
    y1 = sum(f32(c) * t for c, t in zip(coef, t64))
    err = sum(f32(c) * t for c, t in zip(ecoef, t64))
    tol = f32(atol) + f32(rtol) * torch.maximum(t64[0].abs(), y1.abs())
    # what a chain of len(terms) float32 multiply-adds can be off by, element by element: len(terms) 2^-24 sum |c| |t|
    reach = len(terms) * 2.0 ** -24 * sum(abs(f32(c)) * t.abs() for c, t in zip(coef, t64))
    return y1, float(((err / tol) ** 2).sum()), reach


@pytest.mark.parametrize("offset_term", [None, 0, 2])
@pytest.mark.parametrize("nterms", [2, 5, 8])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1048580])
def test_close_kernel_is_the_separate_launches_bit_for_bit(n, nterms, offset_term):
    """y1 torch.equal gode_lincomb_f32's, the sum == gode_rk_errnorm_f32's on that y1, both within float64's reach.  n = 1 048 580:
    more than one grid sweep of the 16-byte form.  offset_term: a term one float past alignment whose error weight is not
    zero, or y0 itself: the scalar form (the third form has the test below)."""
    from graph_odenet_amd import ops
    if offset_term is not None and offset_term >= nterms:
        offset_term = nterms - 1
    terms, coef, ecoef = _close_case(n, nterms, 100 + n % 97 + nterms, offset_term)
    rtol = atol = 1e-3
    y1_ref, s_ref = _separate(terms, coef, ecoef, rtol, atol)
    y1 = torch.empty(n, device=DEV)
    s = ops.rk_close_err_multi([y1], [list(zip(coef, terms))], [ecoef], rtol, atol)
    torch.cuda.synchronize()
    assert torch.equal(y1, y1_ref)
    assert s.item() == s_ref.item(), (s.item(), s_ref.item())
    y64, s64, reach = _float64(terms, coef, ecoef, rtol, atol)
    print("n=%d terms=%d offset=%s: y1 err %.3e, sum %.9e vs float64 %.9e (rel %.3e)"
          % (n, nterms, offset_term, (y1.double().cpu() - y64).abs().max().item(), s.item(), s64, abs(s.item() - s64) / s64))
    assert bool(((y1.double().cpu() - y64).abs() <= reach).all())
    assert abs(s.item() - s64) <= 1e-6 * s64, (s.item(), s64)


ORDERS_SEEN = {}


@pytest.mark.parametrize("nterms", [5, 8])
@pytest.mark.parametrize("n", [4, 1024, 1048580])
def test_close_kernel_keeps_the_16_byte_order_when_only_an_unread_term_is_misaligned(n, nterms):
    """n % 4 == 0 and the ONLY misaligned operand is the term whose error weight is zero: gode_rk_errnorm_f32 does not read
    it and takes its 16-byte form, gode_lincomb_f32 reads it and takes its scalar form.  The close then loads and stores
    scalars but reduces in the 16-byte order (the kernel's third form): y1 and the sum are still the separate launches'
    bits."""
    from graph_odenet_amd import ops
    z = zero_err_term(nterms)
    terms, coef, ecoef = _close_case(n, nterms, 300 + n % 89 + nterms, z)
    assert ecoef[z] == 0.0 and coef[z] != 0.0
    assert all((t.data_ptr() % 16 == 0) != (j == z) for j, t in enumerate(terms))
    rtol = atol = 1e-3
    y1_ref, s_ref = _separate(terms, coef, ecoef, rtol, atol)
    y1 = torch.empty(n, device=DEV)
    s = ops.rk_close_err_multi([y1], [list(zip(coef, terms))], [ecoef], rtol, atol)
    torch.cuda.synchronize()
    assert torch.equal(y1, y1_ref)
    assert s.item() == s_ref.item(), (s.item(), s_ref.item())
    s64 = _float64(terms, coef, ecoef, rtol, atol)[1]
    assert abs(s.item() - s64) <= 1e-6 * s64, (s.item(), s64)
    # the scalar order on the same values (y1 moved one float off alignment: the separate error norm then takes its scalar
    # form) is, on some of these cases, another fp64 number: the comparison above can tell the two orders apart
    y1m = torch.empty(n + 4, device=DEV)[1:n + 1].copy_(y1_ref)
    s_scalar = ops.rk_error_sumsq(terms[0], y1m, [(c, t) for c, t in zip(ecoef, terms) if c != 0.0], rtol, atol)
    print("n=%d terms=%d: sum %.17e, in the scalar order %.17e" % (n, nterms, s.item(), s_scalar.item()))
    ORDERS_SEEN[(n, nterms)] = s_scalar.item() != s.item()
    if len(ORDERS_SEEN) == 6:          # the last case: the two orders are not the same number everywhere (measured: they
        assert any(ORDERS_SEEN.values()), ORDERS_SEEN      # differ at 1 024 x 8 and 1 048 580 x 8, and agree at the other four)


def test_close_kernel_four_components_one_without_output():
    """count = 4 with four different lengths: one component whose only misaligned term carries a zero error weight (the
    16-byte order with scalar loads), one component's y1 NULL, one of length 1, one misaligned on a term the error norm
    reads (the scalar form): every stored y1 and every sum is the single forms'."""
    from graph_odenet_amd import ops
    cases = [_close_case(n, nt, 7 + n, off) for n, nt, off in ((1024, 5, zero_err_term(5)), (4096, 8, None), (1, 2, None),
                                                                (2052, 5, 1))]
    rtol, atol = 1e-3, 1e-5
    outs = [torch.empty(c[0][0].numel(), device=DEV) for c in cases]
    outs[1] = None
    s = ops.rk_close_err_multi(outs, [list(zip(c[1], c[0])) for c in cases], [c[2] for c in cases], rtol, atol)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        y1_ref, s_ref = _separate(*c, rtol, atol)
        if outs[i] is not None:
            assert torch.equal(outs[i], y1_ref), i
        assert s[i].item() == s_ref.item(), i
        s64 = _float64(*c, rtol, atol)[1]
        print("component %d: sum %.9e vs float64 %.9e (rel %.3e)" % (i, s[i].item(), s64, abs(s[i].item() - s64) / s64))
        assert abs(s[i].item() - s64) <= 1e-6 * s64


def test_close_kernel_refuses_aliases():
    from graph_odenet_amd import ops
    terms, coef, ecoef = _close_case(64, 3, 1)
    for j in range(3):
        with pytest.raises(Exception, match="gode_rk_close_err_multi_f32"):
            ops.rk_close_err_multi([terms[j]], [list(zip(coef, terms))], [ecoef], 1e-3, 1e-3)


# ---- 2. the tableau-driven step drivers on dopri5 are the dopri5 drivers ------------------------------------------------------
def gcn_func(d, adj, seed=0, node_order=None):
    from graph_odenet_amd import models
    torch.manual_seed(seed)
    f = models.ODEfunc(d)
    if node_order is not None:
        f.node_order = node_order
    with torch.no_grad():
        f.norm1.weight.uniform_(0.5, 1.5)
        f.norm1.bias.uniform_(-0.5, 0.5)
    f = f.to(DEV)
    f.set_adj(adj if not torch.is_tensor(adj) else adj.to(DEV))
    return f


def gcn_params(f):
    sd = dict(f.named_parameters())
    return [sd[k] for k in R.GCN_PNAMES]


@pytest.mark.parametrize("n,d,small_fused", [(300, 16, 1), (300, 16, 0), (70001, 128, 1)])
def test_new_drivers_on_dopri5_equal_the_dopri5_drivers(n, d, small_fused):
    """GODE_RKA_DOPRI5 through the three new step functions against gode_gcn_ode_dopri5_step_forward / _adjoint / _backprop
    on the same inputs (the fields' members): every output array and every sum under torch.equal.  n = 300, d = 16 on the
    one-launch route and (small_fused 0) the multi-launch one; 70 001 rows, d = 128, 32 groups: the large route."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    adj = R.random_adj(n, 5 * n, 21)
    f = gcn_func(d, adj, seed=3)
    assert f.norm1.num_groups == min(32, d)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(n, d, generator=g).to(DEV)
    t, h, tol = 0.25, 0.3, 1e-3
    old = lib.gode_get_option(b"small_fused")
    lib.gode_set_option(b"small_fused", small_fused)
    try:
        fwd, mk_adj, _ = f.gode_fields(x0)
        fwd.prepare() if fwd.prepare is not None else None
        # forward
        res = {}
        for which in ("old", "new"):
            kk = [[torch.zeros(n, d, device=DEV)] for _ in range(7)]
            fwd.eval(t, [[(1.0, x0)]], kk[0])
            y1 = [torch.empty(n, d, device=DEV)]
            step = fwd.dopri5_step_native if which == "old" else functools.partial(fwd.adaptive_step_native, "dopri5")
            sums = step([x0], kk, y1, t, h, tol, tol)
            torch.cuda.synchronize()
            res[which] = [y1[0]] + [k[0] for k in kk] + [sums]
        assert res["old"][1].abs().max().item() > 1e-2, "k must not be tiny"
        for i, (a, b) in enumerate(zip(res["old"], res["new"])):
            assert torch.equal(a, b), ("forward", i)
        ks = res["old"][1:8]
        # backprop over that step, opening an interval (first) and inside one
        gbar = torch.randn(n, d, generator=g).to(DEV)
        kb7 = torch.randn(n, d, generator=g).to(DEV) * 0.1
        wk = [h * b for b in A.TABLEAUS["dopri5"][2]]
        wk[6] = 0.01 * h
        for first, kbar in ((True, None), (False, kb7)):
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
            for i, (a, b) in enumerate(zip(out["old"], out["new"])):
                assert torch.equal(a, b), ("backprop", first, i)
        # adjoint
        adj_f = mk_adj()
        adj_f.prepare() if adj_f.prepare is not None else None
        res = {}
        for which in ("old", "new"):
            y = adj_f.new_state(x0)
            y[1].copy_(gbar)
            kk = adj_f.alloc_like(y, 7)
            adj_f.eval(t, [[(1.0, c)] for c in y], kk[0])
            (y1,) = adj_f.alloc_like(y, 1)
            step = adj_f.dopri5_step_native if which == "old" else functools.partial(adj_f.adaptive_step_native, "dopri5")
            sums = step(y, kk, y1, t, -h, tol, tol)
            torch.cuda.synchronize()
            res[which] = [y1[0], y1[1], adj_f._theta_of(y1)] + [k[c] for k in kk for c in (0, 1)] + \
                [adj_f._theta_of(k) for k in kk] + [sums]
        assert res["old"][-1].numel() == 4
        for i, (a, b) in enumerate(zip(res["old"], res["new"])):
            assert torch.equal(a, b), ("adjoint", i)
    finally:
        lib.gode_set_option(b"small_fused", old)


# ---- odeint / odeint_adjoint ---------------------------------------------------------------------------------------------------
def product_run(f, x0, t, Rw, method, tol, adjoint, params=None, replay=None):
    """odeint / odeint_adjoint of the product with L = sum_i <y(t_i), Rw_i> -> (outputs, dL/dx0, [dL/dparam], (nfe forward,
    nfe backward), attempt sequences: the forward intervals, then the adjoint solves in the order solved)."""
    from graph_odenet_amd import odeint as OI, solver
    params = list(f.parameters()) if params is None else params
    for p in params:
        p.grad = None
    x = x0.detach().to(DEV).requires_grad_(True)
    if hasattr(f, "nfe"):
        f.nfe = 0
    solve = OI.odeint_adjoint if adjoint else OI.odeint
    solver.TRACE = []
    solver.REPLAY = [list(s) for s in replay] if replay is not None else None
    try:
        out = solve(f, x, torch.tensor(t, device=DEV), rtol=tol, atol=tol, method=method)
        assert out.grad_fn is not None
        nfe_f = getattr(f, "nfe", None)
        if nfe_f is not None:
            f.nfe = 0
        (out * Rw.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        trace = solver.TRACE
    finally:
        solver.TRACE = solver.REPLAY = None
    return out.detach().clone(), x.grad.clone(), [p.grad.clone() for p in params], (nfe_f, getattr(f, "nfe", None)), trace


def check_all(got, refs, what, names):
    (o32, gx32, gp32), (o64, gx64, gp64) = refs
    out, gx, gp = got[:3]
    R.noise_floor_check(out, o32, o64, what + " y(t)")
    R.noise_floor_check(gx, gx32, gx64, what + " dL/dx0")
    assert len(gp) == len(gp64)
    for k, g, g32, g64 in zip(names, gp, gp32, gp64):
        R.noise_floor_check(g.reshape(g64.shape), g32, g64, what + " dL/d" + k)


def refs_for(mk, x0, t, Rw, method, tol, adjoint, trace, params_of=None):
    nf = len(t) - 1
    return A.reference_runs(mk, x0, t, Rw, method, tol, tol, adjoint, trace[:nf], trace[nf:] if adjoint else None,
                            params_of=params_of)


def end_weights(shape, seed, n_t=2):
    Rw = torch.zeros((n_t,) + tuple(shape))
    Rw[-1] = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return Rw


def accepted(seq):
    return [a[0] for a in seq if a[1]]


def last_abscissa(seq, span=1.0):
    acc = accepted(seq)
    return (span - sum(acc[:-1])) / acc[-1]


def cora_adj(golden):
    gr = golden("cora_graph.npz")
    n = int(gr["n"])
    T = lambda a: torch.from_numpy(np.asarray(a))      # noqa: E731
    return torch.sparse_coo_tensor(torch.stack([T(gr["rows"].astype(np.int64)), T(gr["cols"].astype(np.int64))]),
                                   T(gr["vals"]), (n, n)).coalesce()


# ---- 3. bosh3 and adaptive_heun on Cora against float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("adjoint", [True, False])
@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("method", NEW)
def test_cora_vs_float64(golden, method, d, adjoint):
    """Cora, t = [0, 1], rtol = atol = 1e-3, loss <y(1), R>, gcn_func(seed=0), x0 = randn under seed 6: y(1), dL/dx0 and the
    four parameter gradients at the restatement's noise floor through odeint_adjoint and through odeint(adjoint=False), the
    float32 and float64 restatements replaying the product's attempt sequences.  The case has at least two accepted forward
    steps and its last one is cut by the interpolation (asserted; see CASES below for the sequences the CPU restatement
    takes)."""
    adj = cora_adj(golden)
    f = gcn_func(d, adj)
    x0 = torch.randn(adj.shape[0], d, generator=torch.Generator().manual_seed(6))
    Rw = end_weights((adj.shape[0], d), 7)
    got = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, adjoint, params=gcn_params(f))
    seq = got[4][0]
    print("%s d=%d attempts %s" % (method, d, [(round(a[0], 4), a[1]) for a in seq]))
    assert len(accepted(seq)) >= 2 and last_abscissa(seq) < 1.0
    assert len(got[4]) == (2 if adjoint else 1)
    refs = refs_for(lambda dt: R.GcnRef(f, adj, dt), x0, [0.0, 1.0], Rw, method, 1e-3, adjoint, got[4])
    check_all(got, refs, "cora %s d=%d %s" % (method, d, "adjoint" if adjoint else "backprop"), R.GCN_PNAMES)
    S = A.STAGES[method]
    nfe_f = 2 + (S - 1) * len(seq)
    assert got[3][0] == nfe_f
    if adjoint:
        assert got[3][1] == 1 + 2 + (S - 1) * len(got[4][1])      # the dL/dt evaluation, then the adjoint solve's own count
    else:
        assert got[3][1] == 0


# method: (seed of gcn_func, seed of x0, tolerance) of a Cora d = 16 case whose forward solve rejects an attempt.  The float32
# CPU restatement's free-running sequences (|dt|, accepted):
#   bosh3 at 1e-5:         0.0104 T, 0.1044 T, 0.8373 F, 0.2408 T, 1.4834 F, 0.2967 T, 0.4047 T (cut at x = 0.86)
#   adaptive_heun at 1e-3: 0.010 T, 0.103 T, 0.169 T, 0.169 T, 0.198 T, 0.198 F, ... nine attempts, one rejected
#   (adaptive_heun at 1e-5 takes 60 steps on seeds 11 / 12 and rejects none: the case is at 1e-3 on another seed)
# and those of test_cora_vs_float64 (seeds 0 / 6, 1e-3): bosh3 d = 16: 0.0493 T, 0.4928 T, 4.9276 F, 1.7502 F, 1.1048 F,
# 0.9591 T (x = 0.48); bosh3 d = 64: five accepted (x = 0.995); adaptive_heun d = 16 / 64: 8 / 12 accepted (x = 0.10 / 0.10).
REJECTING = {"bosh3": (11, 12, 1e-5), "adaptive_heun": (16, 17, 1e-3)}


@pytest.mark.parametrize("method", NEW)
def test_cora_rejected_attempts(golden, method):
    """Cora d = 16 on the seeds and tolerance of REJECTING: the controller rejects at least one attempt of the forward solve
    (asserted); the rejected attempt leaves no trace in the result or the gradients."""
    adj = cora_adj(golden)
    d = 16
    fseed, xseed, tol = REJECTING[method]
    f = gcn_func(d, adj, seed=fseed)
    x0 = torch.randn(adj.shape[0], d, generator=torch.Generator().manual_seed(xseed))
    Rw = end_weights((adj.shape[0], d), 13)
    for adjoint in (False, True):
        got = product_run(f, x0, [0.0, 1.0], Rw, method, tol, adjoint, params=gcn_params(f))
        seq = got[4][0]
        print("%s attempts %s" % (method, [(round(a[0], 4), a[1]) for a in seq]))
        assert sum(1 for a in seq if not a[1]) >= 1, seq
        refs = refs_for(lambda dt: R.GcnRef(f, adj, dt), x0, [0.0, 1.0], Rw, method, tol, adjoint, got[4])
        check_all(got, refs, "cora rejected %s %s" % (method, "adjoint" if adjoint else "backprop"), R.GCN_PNAMES)


# ---- 4. the one-call step against the per-stage driver -------------------------------------------------------------------------
@pytest.mark.parametrize("method", NEW)
def test_native_step_against_per_stage_driver(method, monkeypatch):
    """n = 300, d = 16: y(1) and the forward attempt sequence agree bit for bit between the one-call step
    (gode_gcn_ode_adaptive_step_*) and the per-stage Python driver (solver.DOPRI5_NATIVE False), the adjoint solve up to the
    summation order of its error sums; recompute mode (BACKPROP_SAVE_MAX_BYTES = 0) gives the gradients of the
    save-everything mode bit for bit."""
    from graph_odenet_amd import odeint as OI, solver
    n, d = 300, 16
    adj = R.random_adj(n, 1500, 31)
    f = gcn_func(d, adj, seed=2)
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(3))
    Rw = end_weights((n, d), 4)
    native = {a: product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, a, params=gcn_params(f)) for a in (True, False)}
    assert len(accepted(native[True][4][0])) >= 2
    monkeypatch.setattr(OI, "BACKPROP_SAVE_MAX_BYTES", 0)
    rec = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, False, params=gcn_params(f))
    assert rec[4] == native[False][4] and torch.equal(rec[0], native[False][0]) and torch.equal(rec[1], native[False][1])
    for a, b in zip(rec[2], native[False][2]):
        assert torch.equal(a, b)
    monkeypatch.setattr(solver, "DOPRI5_NATIVE", False)
    stage = product_run(f, x0, [0.0, 1.0], Rw, method, 1e-3, True, params=gcn_params(f))
    # the forward solve: the same launches, so the same bits.  The adjoint solve: the per-stage driver forms the parameters'
    # error sum per tensor and adds the four, the one-call step sums the packed vector in one reduction - the fp64 sums differ
    # in their last bits (as dopri5's two drivers do, tests/test_gpu_gcn.py), so the same decisions, step sizes equal to
    # 1e-9 and gradients at that test's bars
    assert stage[4][0] == native[True][4][0] and torch.equal(stage[0], native[True][0])
    assert stage[3] == native[True][3]
    sa, sb = stage[4][1], native[True][4][1]
    assert [a[1] for a in sa] == [b[1] for b in sb]
    assert all(abs(a[0] - b[0]) <= 1e-9 * b[0] for a, b in zip(sa, sb))
    R.close(stage[1], native[True][1], 1e-5, method + " per-stage dL/dx0")
    for k, a, b in zip(R.GCN_PNAMES, stage[2], native[True][2]):
        R.close(a, b, 1e-4, method + " per-stage dL/d" + k)


# ---- 5. the large route --------------------------------------------------------------------------------------------------------
def test_large_route_renumbered_bosh3():
    """R-MAT graph of 2^17 rows, d = 128, 32 groups, node_order="degree", bosh3 at rtol = atol = 1e-2: at least two accepted
    steps, the differentiable forward bit for bit the no-grad solve, y(1) and the gradients at the restatement's noise floor."""
    from graph_odenet_amd import odeint as OI, synth
    g = synth.rmat_graph(17, 1 << 20, seed=1, device=DEV)
    rows = torch.repeat_interleave(torch.arange(g.n_rows), (g.rowptr[1:] - g.rowptr[:-1]).cpu().long())
    adj = torch.sparse_coo_tensor(torch.stack([rows, g.col.cpu().long()]), g.val.cpu(), (g.n_rows, g.n_rows)).coalesce()
    d = 128
    f = gcn_func(d, g, seed=4, node_order="degree")
    assert f.norm1.num_groups == 32
    x0 = torch.randn(g.n_rows, d, generator=torch.Generator().manual_seed(5))
    Rw = end_weights((g.n_rows, d), 6)
    got = product_run(f, x0, [0.0, 1.0], Rw, "bosh3", 1e-2, False, params=gcn_params(f))
    assert OI._fields(f, x0.to(DEV))[0].row_order is not None, "the rows must really be renumbered"
    print("attempts %s" % [(round(a[0], 4), a[1]) for a in got[4][0]])
    assert len(accepted(got[4][0])) >= 2
    with torch.no_grad():
        ref = OI.odeint(f, x0.to(DEV), torch.tensor([0.0, 1.0], device=DEV), rtol=1e-2, atol=1e-2, method="bosh3")
    assert torch.equal(got[0], ref), "forward differs from odeint under no_grad"
    refs = refs_for(lambda dt: R.GcnRef(f, adj, dt), x0, [0.0, 1.0], Rw, "bosh3", 1e-2, False, got[4])
    check_all(got, refs, "large bosh3 backprop", R.GCN_PNAMES)


# ---- 6. the other fields: the per-stage driver ----------------------------------------------------------------------------------
@pytest.mark.parametrize("adjoint", [True, False])
def test_generic_func_bosh3(adjoint):
    d, n = 8, 257
    f = R.Mlp(d, seed=3).to(DEV)
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(4))
    Rw = end_weights((n, d), 5)
    got = product_run(f, x0, [0.0, 1.0], Rw, "bosh3", 1e-3, adjoint)
    assert len(accepted(got[4][0])) >= 2
    refs = refs_for(lambda dt: R.Mlp(d, seed=3).to(dt), x0, [0.0, 1.0], Rw, "bosh3", 1e-3, adjoint, got[4])
    check_all(got, refs, "mlp bosh3 %s" % ("adjoint" if adjoint else "backprop"), [k for k, _ in f.named_parameters()])


@pytest.mark.parametrize("adjoint", [True, False])
def test_gat_bosh3(adjoint):
    """The one-head GAT ODE function (n = 300, 1 400 random edges with self loops) on the per-stage driver: its fused evals
    forward and adjoint; adjoint=False takes the generic backprop (the field's seven-stage step members serve dopri5 alone)."""
    from graph_odenet_amd import gat_models
    n, d = 300, 16
    src, tgt = R.random_edges(n, 1400, 17)
    torch.manual_seed(5)
    f = gat_models.ODEfunc(d)
    with torch.no_grad():
        f.norm1.weight.add_(0.3 * torch.randn(d))
        f.norm1.bias.add_(0.3 * torch.randn(d))
    f = f.to(DEV)
    f.set_adj(src.to(DEV), tgt.to(DEV), R.mtgt(n, tgt).to(DEV))
    x0 = 0.5 * torch.randn(n, d, generator=torch.Generator().manual_seed(9))
    Rw = end_weights((n, d), 10)
    fwd = f.gode_fields(x0.to(DEV))[0]
    assert fwd.fused and fwd.adaptive_step_native is None and fwd.adaptive_step_backprop is None
    got = product_run(f, x0, [0.0, 1.0], Rw, "bosh3", 1e-3, adjoint)
    assert len(accepted(got[4][0])) >= 2
    refs = refs_for(lambda dt: R.GatRef(f, n, src, tgt, dt), x0, [0.0, 1.0], Rw, "bosh3", 1e-3, adjoint, got[4])
    check_all(got, refs, "gat bosh3 %s" % ("adjoint" if adjoint else "backprop"), [k for k, _ in f.named_parameters()])


EDGE_KEYS = ("gamma", "beta", "W", "b", "A")


@pytest.mark.parametrize("adjoint", [True, False])
def test_edge_block_bosh3(adjoint):
    """EdgeODEBlock(method='bosh3') on 20 small molecules' worth of random edges, h = 16: forward, adjoint and (adjoint=False)
    the generic backprop, the edge matrices' gradient included."""
    from graph_odenet_amd import solver
    from test_gpu_qc_ode import batch_of, block_run, product
    from test_qc_ode_api import RefEdgeODEfunc
    h = 16
    x0, Esrc, etgt, val, Am, _ = batch_of(20, h, seed=7)
    f, Ad = product(h, Esrc, etgt, val, Am)
    Rw = end_weights(x0.shape, 4)
    solver.TRACE = []
    try:
        got, nfe = block_run(f, Ad, x0, Rw[1], "bosh3", None, tol=1e-3, adjoint=adjoint)
        torch.cuda.synchronize()
        trace = solver.TRACE
    finally:
        solver.TRACE = None
    assert len(trace) == (2 if adjoint else 1) and len(accepted(trace[0])) >= 2
    pair = {dt: RefEdgeODEfunc(h, Esrc, etgt, val, Am, dtype=dt).load(f) for dt in (torch.float32, torch.float64)}
    (o32, gx32, gp32), (o64, gx64, gp64) = refs_for(lambda dt: pair[dt], x0, [0.0, 1.0], Rw, "bosh3", 1e-3, adjoint, trace,
                                                    params_of=lambda r: [getattr(r, k) for k in EDGE_KEYS])
    what = "edge bosh3 %s" % ("adjoint" if adjoint else "backprop")
    R.noise_floor_check(got["y"], o32[1], o64[1], what + " y(1)")
    R.noise_floor_check(got["x"], gx32, gx64, what + " dL/dx0")
    for i, k in enumerate(EDGE_KEYS):
        R.noise_floor_check(got[k], gp32[i], gp64[i], what + " dL/d" + k)
    assert nfe[0] == 2 + 3 * len(trace[0])


# ---- 7. the remaining paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", NEW)
def test_three_output_times_and_nfe(method):
    """t = [0, 0.4, 1] with a cotangent on every output: three outputs matching the restatement through both gradient paths;
    stats.nfe = 2 + (S - 1) attempts per interval, and func.nfe agrees."""
    n, d = 300, 16
    adj = R.random_adj(n, 1500, 31)
    f = gcn_func(d, adj, seed=2)
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(3))
    t = [0.0, 0.4, 1.0]
    Rw = torch.randn((3, n, d), generator=torch.Generator().manual_seed(8))
    S = A.STAGES[method]
    for adjoint in (False, True):
        got = product_run(f, x0, t, Rw, method, 1e-3, adjoint, params=gcn_params(f))
        assert got[0].shape[0] == 3 and torch.equal(got[0][0].cpu(), x0)
        trace = got[4]
        assert len(trace) == (4 if adjoint else 2)
        assert got[3][0] == sum(2 + (S - 1) * len(s) for s in trace[:2])
        if adjoint:
            assert got[3][1] == sum(1 + 2 + (S - 1) * len(s) for s in trace[2:])
        refs = refs_for(lambda dt: R.GcnRef(f, adj, dt), x0, t, Rw, method, 1e-3, adjoint, trace)
        check_all(got, refs, "3 times %s %s" % (method, "adjoint" if adjoint else "backprop"), R.GCN_PNAMES)


@pytest.mark.parametrize("method", ["dopri5"] + NEW)
def test_free_running_controller_takes_the_restatements_steps(method):
    """No replay: the product's own initial step and controller (exponent 1/p in both) against the float32 restatement's
    on a smooth func (the tanh MLP, 257 x 8, rtol = atol = 1e-4) - the first attempted step of the forward solve (one tensor)
    and of the adjoint solve (four error groups) within 2e-3, the bar tests/test_gpu_gcn.py sets for dopri5's first steps,
    and the forward solve's whole attempt sequence: the same decisions, every step size within 2e-3."""
    d, n, tol = 8, 257, 1e-4
    f = R.Mlp(d, seed=3).to(DEV)
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(4))
    Rw = end_weights((n, d), 5)
    got = product_run(f, x0, [0.0, 1.0], Rw, method, tol, True)
    ref = R.Mlp(d, seed=3)
    out, seqs_f, _ = A.odeint(ref, x0, [0.0, 1.0], method, tol, tol)
    _, _, seqs_b = A.adjoint_grads(ref, list(ref.parameters()), out, [0.0, 1.0], Rw, method, tol, tol)
    for k, (mine, theirs) in enumerate(((got[4][0], seqs_f[0]), (got[4][1], seqs_b[0]))):
        print("%s solve %d: product %s" % (method, k, [(round(a[0], 5), a[1]) for a in mine]))
        print("%s solve %d: restatement %s" % (method, k, [(round(a[0], 5), a[1]) for a in theirs]))
        assert abs(mine[0][0] - theirs[0][0]) <= 2e-3 * theirs[0][0], (k, mine[0], theirs[0])
    mine, theirs = got[4][0], seqs_f[0]
    assert [a[1] for a in mine] == [a[1] for a in theirs]
    assert all(abs(a[0] - b[0]) <= 2e-3 * b[0] for a, b in zip(mine, theirs))


def test_fixed_grid_only_fields_refuse_the_new_methods():
    from graph_odenet_amd import odeint as OI, solver

    class Fixed(solver.Field):
        fixed_grid_only = True
    for m in NEW:
        with pytest.raises(NotImplementedError):
            OI._integrate(Fixed(), [torch.zeros(2, device=DEV)], 0.0, 1.0, 1e-3, 1e-3, m, None, solver.Dopri5Stats())


def test_ode_block_trains_under_bosh3(golden):
    """ODEGCN3 with ODEBlock(method='bosh3') on Cora: three Adam steps, the loss finite and decreasing."""
    from graph_odenet_amd import models
    adj = cora_adj(golden)
    n = adj.shape[0]
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(n, 32, generator=g).to(DEV)
    labels = torch.randint(0, 7, (n,), generator=g).to(DEV)
    torch.manual_seed(1)
    m = models.ODEGCN3(nfeat=32, nhid=16, nclass=7, dropout=0.0, method="bosh3", tol=1e-3).to(DEV)
    assert m.gc2.method == "bosh3"
    opt = torch.optim.Adam(m.parameters(), lr=0.01)
    adj_dev = adj.to(DEV)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(m(feats, adj_dev), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0]
    assert m.nfe > 0
