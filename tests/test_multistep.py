"""explicit_adams (4th-order Adams-Bashforth, rk4 start-up) without a GPU: the coefficients' order conditions, the order and
the start-up of the float64 restatement the GPU tests compare against (tests/multistep_ref.py), the evaluation count, the
validation codes of the new entry points (they come back before any HIP call; pointers that must never be dereferenced are
dummies), the record layout query, and the names odeint, the fields and the two CLIs accept."""
import ctypes

import pytest
import torch

import fixed_methods_ref as R
import multistep_ref as M
from graph_odenet_amd import _lib

E_NULLPTR, E_SHAPE, E_UNSUPPORTED = -1, -2, -5
DUMMY = ctypes.c_void_p(256)          # a non-NULL device address the validation never touches


# ---- the method -------------------------------------------------------------------------------------------------------------
def test_coefficients_meet_the_order_conditions():
    """sum beta = 1 and sum_j beta_j (-j)^k = 1 / (k + 1) for k = 0..3: the quadrature of the cubic through f_i .. f_{i-3} over
    [t_i, t_i + h] - in the product's table, the restatement's and the C drivers' (through their record of the weights)."""
    from graph_odenet_amd import solver
    assert solver.MULTISTEP_METHODS == ("explicit_adams",)
    assert tuple(solver.MULTISTEP_BETAS["explicit_adams"]) == M.BETA == tuple(solver.ADAMS_BETA)
    for beta in (M.BETA, solver.ADAMS_BETA):
        assert len(beta) == 4 and abs(sum(beta) - 1.0) < 1e-15
        for k in range(4):
            assert abs(sum(b * float(-j) ** k for j, b in enumerate(beta)) - 1.0 / (k + 1)) < 1e-14, k
        assert abs(sum(b * float(-j) ** 4 for j, b in enumerate(beta)) - 1.0 / 5) > 1.0   # and not the fifth: 251/720 * 4!


def test_restatement_is_fourth_order():
    """fixed_methods_ref.Mlp(8) in float64, a 32 x 8 state over [0, 1], against rk4 at 4096 steps: halving h must divide the
    maximum error by a factor in (12, 28) for n = 32 -> 64 and 64 -> 128 - order 3 gives 8, order 5 gives 32.  The state is
    the draw the GPU tests' MLP case uses (generator seed 4).  Measured: errors 3.9e-4, 4.6e-5, 3.2e-6, 2.0e-7 at n = 16, 32,
    64, 128 (ratios 14.5 and 16.0; rk4 on the same grids 2.7e-6 .. 6.8e-10).  On y' = -y the ratios are 15.6 and 15.8.  The
    maximum over one state's 256 elements scatters at these step sizes - over 18 other draws the 32 -> 64 ratio ranged from
    9.8 to 31.5, the 64 -> 128 ratio from 13.0 to 19.5 - so the linear problem is held to the tighter (15, 17)."""
    f = R.Mlp(8).double()
    y0 = torch.randn(32, 8, generator=torch.Generator().manual_seed(4)).double()
    with torch.no_grad():
        ref = R.solve(f, y0, 0.0, 1.0, 4096, "rk4")
        err = {n: (M.solve(f, y0, 0.0, 1.0, n) - ref).abs().max().item() for n in (16, 32, 64, 128)}
    print("errors", err, "ratios %.2f %.2f" % (err[32] / err[64], err[64] / err[128]))
    assert 12 < err[32] / err[64] < 28 and 12 < err[64] / err[128] < 28
    one = torch.ones(1, dtype=torch.float64)
    lin = {n: (M.solve(lambda t, y: -y, one, 0.0, 1.0, n) - torch.exp(-one)).abs().item() for n in (32, 64, 128)}
    assert 15 < lin[32] / lin[64] < 17 and 15 < lin[64] / lin[128] < 17


@pytest.mark.parametrize("n", [1, 2, 3])
def test_start_up_only_is_rk4(n):
    """n <= 3: the solve is the rk4 restatement's, exactly - outputs, autograd gradients and adjoint gradients."""
    f = R.Mlp(8, seed=1).double()
    y0 = torch.randn(5, 8, generator=torch.Generator().manual_seed(2)).double()
    Rw = torch.randn(2, 5, 8, generator=torch.Generator().manual_seed(3)).double()
    mk = lambda dt: R.Mlp(8, seed=1).to(dt)      # noqa: E731
    for adjoint in (False, True):
        for a, b in zip(M.reference_runs(mk, y0, [0.0, 1.0], Rw, 1.0 / n, adjoint),
                        R.reference_runs(mk, y0, [0.0, 1.0], Rw, "rk4", 1.0 / n, adjoint)):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert all(torch.equal(u, v) for u, v in zip(a[2], b[2]))
    with torch.no_grad():
        assert not torch.equal(M.solve(f, y0, 0.0, 1.0, 4), R.solve(f, y0, 0.0, 1.0, 4, "rk4"))


def test_nfe_formula():
    """E(n) = 4 min(n, 3) + max(n - 3, 0): counted on the restatement, stated by the product (16 steps: 25 against rk4's 64)."""
    from graph_odenet_amd import odeint as OI, solver
    for n in (1, 2, 3, 4, 5, 7, 16):
        calls = []

        def f(t, y):
            calls.append(float(t))
            return -y
        M.solve(f, torch.ones(2, dtype=torch.float64), 0.0, 1.0, n)
        assert len(calls) == M.nfe(n) == solver.multistep_nfe("explicit_adams", n) == OI._grid_nfe("explicit_adams", n)
        assert calls[-1] == pytest.approx((n - 1) / n if n > 3 else 1.0)
    assert M.nfe(16) == 25 and OI._grid_nfe("rk4", 16) == 64 and OI._grid_nfe("midpoint", 16) == 32


def test_quadrature_weights_sum_the_history():
    """solver.multistep_weight: the weight f_i ends up with over the multistep steps that read it.  Summed over i, with the
    start-up steps' h, it is the length of the interval (the method integrates a constant exactly)."""
    from graph_odenet_amd import solver
    for n in (4, 5, 7, 16):
        h = 1.0 / n
        w = [solver.multistep_weight("explicit_adams", i, n, h) for i in range(n)]
        assert abs(sum(w) + 3 * h - 1.0) < 1e-14
        for i in range(n):
            reads = [m - i for m in range(max(i, 3), n) if m - i <= 3]
            assert abs(w[i] - h * sum(M.BETA[j] for j in reads)) < 1e-15
        if n >= 7:
            assert abs(w[3] - h) < 1e-15                 # read by four steps with all four weights


def test_python_driver_on_a_cpu_field_matches_the_restatement(monkeypatch):
    """solver.integrate_multistep on a field with plain torch arithmetic (the RK kernels replaced by their definition):
    n = 4, 7 against the restatement in float64; the deferral protocol - a quadrature component advanced by finish_rk4_step
    with each evaluation's final weight - gives the same integral as the history does."""
    from graph_odenet_amd import solver

    def lincomb_(out, terms):
        out.copy_(sum(c * x for c, x in terms))
        return out
    monkeypatch.setattr(solver.ops, "lincomb_", lincomb_)
    monkeypatch.setattr(solver.ops, "lincomb_multi_", lambda outs, terms: [lincomb_(o, t) for o, t in zip(outs, terms)])
    w = torch.tensor([[-0.7, 0.4], [0.3, -0.9]], dtype=torch.float64)

    def rhs(t, y):
        return torch.tanh(y @ w) * (1.0 + t)

    class F(solver.Field):
        """(y, q): q' = sum(y^2) is a pure quadrature."""
        n_components = 2
        defer = False
        deferred_components = (1,)

        def __init__(self):
            self.pending, self.calls = None, 0

        def eval(self, t, terms, out):
            y = sum(c * x for c, x in terms[0])
            out[0].copy_(rhs(t, y))
            self.calls += 1
            if self.pending is not None:
                self.pending.append((y * y).sum().reshape(1))
            else:
                out[1].copy_((y * y).sum().reshape(1))

        def begin_rk4_step(self):
            self.pending = [] if self.defer else None
            return self.defer

        def finish_rk4_step(self, weights, y):
            assert len(weights) >= len(self.pending)
            y[1].add_(sum(wt * v for wt, v in zip(weights, self.pending)))
            self.pending = None
            return self.deferred_components

    y0 = torch.tensor([[0.3, -1.1], [0.8, 0.2], [-0.5, 0.9]], dtype=torch.float64)
    for n in (2, 4, 7):
        ref = M.solve(lambda t, s: (rhs(float(t), s[0]), (s[0] * s[0]).sum().reshape(1)), (y0, torch.zeros(1, dtype=torch.float64)),
                      0.0, 1.0, n)
        for defer in (False, True):
            fld = F()
            fld.defer = defer
            y = [y0.clone(), torch.zeros(1, dtype=torch.float64)]
            nfe = solver.integrate_multistep(fld, y, 0.0, 1.0, n, "explicit_adams")
            assert nfe == fld.calls == M.nfe(n)
            assert (y[0] - ref[0]).abs().max().item() < 1e-14 and abs(y[1].item() - ref[1].item()) < 1e-13, (n, defer)


# ---- validation codes through the ABI ------------------------------------------------------------------------------------------
def gcn_structs(n=8, d=16, groups=16):
    f = _lib.GcnOdeFunc()
    f.n, f.d, f.groups, f.eps = n, d, groups, 1e-5
    return f, _lib.Rk4Workspace()


def test_entry_points_are_bound_from_the_header():
    lib = _lib.load()
    for name in ("gode_gcn_ode_adams_forward", "gode_gcn_ode_adams_adjoint", "gode_gcn_ode_adams_forward_save",
                 "gode_gcn_ode_adams_backprop", "gode_adams_record_offset", "gode_gcn_feval_small_save_cot_f32",
                 "gode_gcn_vjp_small_raw_f32"):
        assert callable(getattr(lib, name)), name
    assert len(_lib.STRUCTS) == 11                                     # history and work arrays ride as pointer arguments
    assert "GODE_RK_EXPLICIT_ADAMS" not in _lib.CONSTANTS              # the method has no GODE_RK_* code ...
    assert lib.gode_rk_stages(3) == E_SHAPE and lib.gode_rk_tableau(3, None, None, None) == E_SHAPE
    f, ws = gcn_structs()
    res = ctypes.c_void_p()
    assert lib.gode_gcn_ode_fixed_forward(3, ctypes.byref(f), DUMMY, ctypes.byref(res), ctypes.byref(ws), 0.0, 1.0, 4, None) == E_SHAPE
    assert lib.gode_gcn_ode_fixed_adjoint(3, ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(res), ctypes.byref(res),
                                          ctypes.byref(ws), 0.0, 1.0, 4, None) == E_SHAPE
    assert lib.gode_gcn_ode_fixed_forward_save(3, ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(ws), 0.0, 1.0, 4, 0, 4, None) == E_SHAPE
    assert lib.gode_gcn_ode_fixed_backprop(3, ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(res), ctypes.byref(ws), None,
                                           0.0, 1.0, 4, 0, 4, None) == E_SHAPE


def test_forward_validation():
    """Null arguments, then shapes, then the members of ws and extra; n_steps <= 3 goes through rk4's own checks."""
    fwd = _lib.load().gode_gcn_ode_adams_forward
    f, ws = gcn_structs()
    res = ctypes.c_void_p()
    extra = (ctypes.c_void_p * 2)(256, 256)
    ok = lambda n=5, ff=f, w=ws, ex=extra: [ctypes.byref(ff), DUMMY, ctypes.byref(res), ctypes.byref(w), ex, 0.0, 1.0, n, None]   # noqa: E731
    for i in (0, 1, 2, 3, 4):
        a = ok()
        a[i] = None
        assert fwd(*a) == E_NULLPTR, i
    a = ok(n=0)
    a[1] = None
    assert fwd(*a) == E_NULLPTR                                        # null pointers come first
    assert fwd(*ok(n=0)) == E_SHAPE and fwd(*ok(n=-2)) == E_SHAPE
    assert fwd(*ok(ff=gcn_structs(n=0)[0])) == E_SHAPE and fwd(*ok(ff=gcn_structs(d=0)[0])) == E_SHAPE
    assert fwd(*ok()) == E_NULLPTR                                     # ws->S
    assert fwd(*ok(n=3)) == E_NULLPTR                                  # rk4 through the same door: its own ws check
    full = _lib.Rk4Workspace()
    full.S = 256
    for i in range(4):
        full.ky[i] = 256
    assert fwd(*ok(w=full, ex=(ctypes.c_void_p * 2)(256, None))) == E_NULLPTR      # an entry of extra


def test_adjoint_validation():
    """Null arguments, then shapes, then the route (GODE_E_UNSUPPORTED off the launch-bound route), then ws and extra."""
    adj = _lib.load().gode_gcn_ode_adams_adjoint
    yr, ar = ctypes.c_void_p(), ctypes.c_void_p()
    extra = (ctypes.c_void_p * 4)(256, 256, 256, 256)

    def ok(n=5, ff=None, ws=None, ex=extra):
        ff = gcn_structs()[0] if ff is None else ff
        ws = gcn_structs()[1] if ws is None else ws
        return [ctypes.byref(ff), DUMMY, DUMMY, DUMMY, ctypes.byref(yr), ctypes.byref(ar), ctypes.byref(ws), ex, 0.0, 1.0, n, None]
    for i in range(8):
        a = ok()
        a[i] = None
        assert adj(*a) == E_NULLPTR, i
    assert adj(*ok(n=0)) == E_SHAPE and adj(*ok(ff=gcn_structs(n=0)[0])) == E_SHAPE
    assert adj(*ok()) == E_UNSUPPORTED                                 # no small_part: not the launch-bound route
    assert adj(*ok(n=2)) == E_UNSUPPORTED                              # ... whatever the step count
    ws = _lib.Rk4Workspace()
    ws.small_part = 256
    assert adj(*ok(ws=ws)) == E_NULLPTR                                # on the route: the stage buffers are missing
    assert adj(*ok(ws=ws, ff=gcn_structs(n=65537)[0])) == E_UNSUPPORTED            # above the one-launch kernels' rows
    assert adj(*ok(ws=ws, ff=gcn_structs(d=128, groups=32)[0])) == E_UNSUPPORTED   # and beside their widths
    assert adj(*ok(ws=ws, ff=gcn_structs(n=0)[0])) == E_SHAPE                      # shapes before the route
    for i in range(4):
        ws.ky[i] = ws.ka[i] = 256
    assert adj(*ok(ws=ws)) == E_NULLPTR                                # ws->dZ
    ws.dZ = 256
    assert adj(*ok(ws=ws, ex=(ctypes.c_void_p * 4)(256, 256, 256, None))) == E_NULLPTR


def test_forward_save_and_backprop_validation():
    """Null arguments, then shapes and step ranges, then the members of ws, hist and work."""
    lib = _lib.load()
    f, ws = gcn_structs()
    fwd = lib.gode_gcn_ode_adams_forward_save
    ok = lambda st=(7, 0, 7), ff=f, w=ws, hist=None: [ctypes.byref(ff), DUMMY, DUMMY, DUMMY, hist, ctypes.byref(w), 0.0, 1.0, st[0], st[1], st[2], None]   # noqa: E731
    for i in (0, 1, 2, 3, 5):
        a = ok()
        a[i] = None
        assert fwd(*a) == E_NULLPTR, i
    a = ok(st=(0, 0, 1))
    a[1] = None
    assert fwd(*a) == E_NULLPTR                                        # null pointers come first
    assert fwd(*ok(st=(0, 0, 1))) == E_SHAPE                           # no steps
    assert fwd(*ok(st=(7, 2, 2))) == E_SHAPE                           # empty range
    assert fwd(*ok(st=(7, 5, 1))) == E_SHAPE                           # out of order
    assert fwd(*ok(st=(7, 0, 8))) == E_SHAPE                           # past the grid
    assert fwd(*ok(ff=gcn_structs(n=0)[0])) == E_SHAPE
    assert fwd(*ok()) == E_NULLPTR                                     # ws->S
    assert fwd(*ok(st=(3, 0, 3))) == E_NULLPTR                         # rk4 through the same door: its own ws check
    has_s = _lib.Rk4Workspace()
    has_s.S = 256
    assert fwd(*ok(st=(7, 4, 7), w=has_s)) == E_NULLPTR                # a multistep step from step 4 on needs the history
    assert fwd(*ok(st=(7, 4, 7), w=has_s, hist=(ctypes.c_void_p * 3)(256, None, 256))) == E_NULLPTR
    bp = lib.gode_gcn_ode_adams_backprop
    res = ctypes.c_void_p()
    work = (ctypes.c_void_p * 4)(256, 256, 256, 256)

    def okb(n=7, ff=f, w=None, wk=work, rerun=None):
        w = _lib.Rk4Workspace() if w is None else w
        return [ctypes.byref(ff), DUMMY, rerun, DUMMY, DUMMY, ctypes.byref(res), ctypes.byref(w), None, wk, 0.0, 1.0, n, None]
    for i in (0, 1, 3, 4, 5, 6, 8):
        a = okb()
        a[i] = None
        assert bp(*a) == E_NULLPTR, i
    assert bp(*okb(n=0)) == E_SHAPE and bp(*okb(ff=gcn_structs(d=0)[0])) == E_SHAPE
    assert bp(*okb(n=3, rerun=DUMMY)) == E_SHAPE                       # three steps are rk4's: its re-run mode is the caller's
    assert bp(*okb()) == E_NULLPTR                                     # the stage buffers
    assert bp(*okb(n=3)) == E_NULLPTR                                  # rk4 through the same door
    ws2 = _lib.Rk4Workspace()
    for i in range(4):
        ws2.ka[i] = ws2.ktheta[i] = 256
    assert bp(*okb(w=ws2, wk=(ctypes.c_void_p * 4)(256, 256, None, 256))) == E_NULLPTR
    ws2.dZ = ws2.dS = 256
    assert bp(*okb(w=ws2)) == E_NULLPTR                                # the partial buffers still missing


def test_record_offsets_are_the_layout():
    """A start-up step keeps [y | k_1..k_4] (5 nd floats), a multistep step [y | f] (2 nd): the host query against the
    restatement's statement of the layout, and the totals the sizes in the documents come from."""
    lib = _lib.load()
    from graph_odenet_amd import gcn_ode
    for nd in (1, 257 * 16):
        for n in (1, 3, 4, 7, 16):
            for step in range(n + 1):
                want = M.record_floats(n, step, nd)
                assert lib.gode_adams_record_offset(step, nd) == want
                assert gcn_ode.GcnOdeField.multistep_record_floats("explicit_adams", n, step, nd) == want
    assert [lib.gode_adams_record_offset(s, 10) for s in range(6)] == [0, 50, 100, 150, 170, 190]
    assert lib.gode_adams_record_offset(-1, 10) == E_SHAPE and lib.gode_adams_record_offset(2, -1) == E_SHAPE
    nd = (1 << 20) * 128
    assert round(lib.gode_adams_record_offset(16, nd) * 4 / 1e9) == 22 and round(16 * 5 * nd * 4 / 1e9) == 43


def test_one_launch_forms_validation():
    """The two forms a multistep adjoint step is made of: null outputs, aliased outputs, then the route."""
    lib = _lib.load()
    f, _ = gcn_structs()
    lc = _lib.LinComb()
    lc.n, lc.coef[0], lc.ptr[0] = 1, 1.0, 4096
    sc = lib.gode_gcn_feval_small_save_cot_f32
    B = [ctypes.c_void_p(4096 + 1024 * i) for i in range(1, 5)]
    assert sc(ctypes.byref(f), ctypes.byref(lc), 0.0, 1.0, None, None, B[0], B[1], B[2], None) == E_NULLPTR      # cot
    assert sc(ctypes.byref(f), ctypes.byref(lc), 0.0, 1.0, None, ctypes.byref(lc), None, B[1], B[2], None) == E_NULLPTR   # Y2
    assert sc(ctypes.byref(f), ctypes.byref(lc), 0.0, 1.0, None, ctypes.byref(lc), B[0], B[1], None, None) == E_NULLPTR   # k
    assert sc(ctypes.byref(f), ctypes.byref(lc), 0.0, 1.0, None, ctypes.byref(lc), B[0], B[0], B[2], None) == E_SHAPE     # Y2 = out
    assert sc(ctypes.byref(f), ctypes.byref(lc), 0.0, 1.0, None, ctypes.byref(lc), B[0], B[1], B[1], None) == E_SHAPE     # k = out
    f128 = gcn_structs(d=128, groups=32)[0]
    assert sc(ctypes.byref(f128), ctypes.byref(lc), 0.0, 1.0, None, ctypes.byref(lc), B[0], B[1], B[2], None) == E_UNSUPPORTED
    vr = lib.gode_gcn_vjp_small_raw_f32
    assert vr(ctypes.byref(f), ctypes.byref(lc), B[0], 1.0, None, B[1], B[2], None, None) == E_NULLPTR           # raw
    assert vr(ctypes.byref(f), ctypes.byref(lc), B[0], 1.0, None, B[1], B[2], B[1], None) == E_SHAPE             # raw = ka
    assert vr(ctypes.byref(f), ctypes.byref(lc), B[0], 1.0, None, B[1], B[2], B[0], None) == E_SHAPE             # raw = dZ
    assert vr(ctypes.byref(f128), ctypes.byref(lc), B[0], 1.0, None, B[1], B[2], B[3], None) == E_UNSUPPORTED


# ---- the names ----------------------------------------------------------------------------------------------------------------
def test_method_names():
    from graph_odenet_amd import odeint as OI, solver
    assert OI.METHODS == ("dopri5", "rk4", "euler", "midpoint", "bosh3", "adaptive_heun")
    assert solver.FIXED_METHODS == ("rk4", "euler", "midpoint") and tuple(solver.FIXED_TABLEAUS) == solver.FIXED_METHODS
    assert OI._method("explicit_adams") == "explicit_adams" and OI._method(None) == "dopri5"
    for m in ("adams", "tsit5", "Explicit_Adams", "explicit-adams", ""):
        with pytest.raises(ValueError, match="dopri5, rk4, euler, midpoint, bosh3, adaptive_heun, explicit_adams"):
            OI._method(m)
    with pytest.raises(KeyError):
        solver.n_stages("explicit_adams")                # no tableau, no GODE_RK_* code
    with pytest.raises(ValueError):
        solver.method_code("explicit_adams")


def test_start_up_only_grids_run_as_rk4():
    """A grid of at most three steps per interval is handed to the rk4 paths whole; a longer interval keeps the method."""
    from graph_odenet_amd import odeint as OI
    assert OI._grid_method("explicit_adams", [0.0, 1.0], {"step_size": 1 / 3}) == "rk4"
    assert OI._grid_method("explicit_adams", [0.0, 1.0], None) == "rk4"
    assert OI._grid_method("explicit_adams", [0.0, 1.0], {"step_size": 0.25}) == "explicit_adams"
    assert OI._grid_method("explicit_adams", [0.0, 0.3, 1.0], {"step_size": 0.1}) == "explicit_adams"
    assert OI._grid_method("euler", [0.0, 1.0], {"step_size": 0.5}) == "euler"


def test_clis_accept_the_method():
    from graph_odenet_amd import train_layers, train_res
    for mod in (train_res, train_layers):
        a = mod.build_parser().parse_args(["--method", "explicit_adams", "--step_size", "0.0625"])
        assert a.method == "explicit_adams" and a.step_size == 0.0625
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--method", "adams"])


def test_fields_offer_the_protocol_members():
    from graph_odenet_amd import gcn_ode, solver
    for name in ("multistep_native", "multistep_forward_save", "multistep_backprop"):
        assert getattr(solver.Field, name) is None
    assert callable(gcn_ode.GcnOdeField.multistep_native) and callable(gcn_ode.GcnOdeAdjointField.multistep_native)
    assert callable(gcn_ode.GcnOdeField.multistep_forward_save) and callable(gcn_ode.GcnOdeField.multistep_backprop)
    assert gcn_ode.GcnOdePartField.multistep_native is None and gcn_ode.GcnOdePartAdjointField.multistep_native is None
    assert gcn_ode.GcnOdePartField.multistep_forward_save is None and gcn_ode.GcnOdePartField.multistep_backprop is None
    for mod, cls in (("gat_ode", "GatOdeField"), ("qc_ode", "EdgeOdeField")):        # these run on the Python driver
        fld = getattr(__import__("graph_odenet_amd." + mod, fromlist=[cls]), cls)
        assert fld.multistep_native is None and fld.multistep_forward_save is None
    assert callable(solver.integrate_multistep)
