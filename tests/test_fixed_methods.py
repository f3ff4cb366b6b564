"""The fixed-grid methods euler and midpoint without a GPU: the tableaus of solver.py against the C drivers' (gode_rk_stages /
gode_rk_tableau), the orders of the float64 restatement the GPU tests compare against (tests/fixed_methods_ref.py), the
validation codes of every new entry point (they come back before any HIP call; pointers that must never be dereferenced are
dummies), and the names odeint and the two CLIs accept."""
import ctypes
import math

import pytest
import torch

import fixed_methods_ref as R
from graph_odenet_amd import _lib

E_NULLPTR, E_SHAPE, E_UNSUPPORTED = -1, -2, -5
DUMMY = ctypes.c_void_p(256)          # a non-NULL device address the validation never touches
EULER, MIDPOINT = 1, 2
P = ctypes.addressof


# ---- tableaus ---------------------------------------------------------------------------------------------------------------
def test_tableaus_are_consistent_and_the_c_tables_are_pythons():
    from graph_odenet_amd import solver
    lib = _lib.load()
    assert _lib.CONSTANTS["GODE_RK_RK4_38"] == 0 and _lib.CONSTANTS["GODE_RK_EULER"] == 1 and _lib.CONSTANTS["GODE_RK_MIDPOINT"] == 2
    assert solver.FIXED_METHODS == ("rk4", "euler", "midpoint")
    for code, name in enumerate(solver.FIXED_METHODS):
        c, a, b = solver.FIXED_TABLEAUS[name]
        S = len(c)
        assert solver.method_code(name) == code == R.CODES[name] and solver.n_stages(name) == S
        assert len(a) == S and len(b) == S and all(len(a[s]) <= s for s in range(S))
        assert abs(sum(b) - 1.0) < 1e-15
        for s in range(S):
            assert abs(c[s] - sum(a[s])) < 1e-15, (name, s)
        assert (c, a, b) == tuple(R.TABLEAUS[name]), name              # the restatement's own statement of them
        assert lib.gode_rk_stages(code) == S
        cc, bb, aa = (ctypes.c_double * S)(), (ctypes.c_double * S)(), (ctypes.c_double * (S * S))()
        assert lib.gode_rk_tableau(code, cc, aa, bb) == 0
        assert list(cc) == c and list(bb) == b
        for s in range(S):
            assert list(aa[s * S:(s + 1) * S]) == list(a[s]) + [0.0] * (S - len(a[s])), (name, s)
        assert lib.gode_rk_tableau(code, None, None, None) == 0
    for bad in (-1, 3):
        assert lib.gode_rk_stages(bad) == E_SHAPE
        assert lib.gode_rk_tableau(bad, None, None, None) == E_SHAPE
    assert solver.FIXED_TABLEAUS["midpoint"][2][0] == 0.0              # b_1 = 0: the closing combination never reads k_1


@pytest.mark.parametrize("method,lo,hi", [("euler", 1.8, 2.3), ("midpoint", 3.6, 4.5)])
def test_restatement_has_the_order_it_should(method, lo, hi):
    """y' = -y over [0, 1] in float64 at h = 1/8, then 1/16: the error ratio is 2.06 for euler ((1 - h)^(1/h) against 1/e) and
    4.19 for midpoint ((1 - h + h^2 / 2)^(1/h))."""
    y0 = torch.ones(3, dtype=torch.float64)
    errs = []
    for n in (8, 16):
        y = R.solve(lambda t, y: -y, y0, 0.0, 1.0, n, method)
        errs.append((y - math.exp(-1.0)).abs().max().item())
    ratio = errs[0] / errs[1]
    print("%s: errors %.6e %.6e ratio %.4f" % (method, errs[0], errs[1], ratio))
    assert lo <= ratio <= hi
    growth = {"euler": lambda h: 1 - h, "midpoint": lambda h: 1 - h + h * h / 2}[method]
    assert abs(R.solve(lambda t, y: -y, y0, 0.0, 1.0, 8, method)[0].item() - growth(1 / 8) ** 8) < 1e-15


def test_restatement_adjoint_of_a_linear_field_is_exact_algebra():
    """For y' = w y the discrete adjoint of either method multiplies a by the same growth factor as y per step, and
    dL/dw accumulates through the augmented state: checked against autograd through the forward restatement for euler,
    where the two coincide (one stage, the adjoint's stage is evaluated at y_{n+1} going backwards - so they differ at
    O(h); the test pins the value by hand instead)."""
    w = torch.nn.Parameter(torch.tensor(0.5, dtype=torch.float64))
    y0 = torch.tensor([2.0], dtype=torch.float64)
    f = lambda t, y: w * y                                             # noqa: E731
    out = R.odeint(f, y0, [0.0, 1.0], "euler", 0.5)
    assert abs(out[1].item() - 2.0 * 1.25 ** 2) < 1e-15
    ga, (gw,) = R.adjoint_grads(f, [w], out, [0.0, 1.0], torch.ones_like(out), "euler", 0.5)
    # backwards, h = -1/2: a <- a - h w a = 1.25 a per step, twice, plus the cotangent of y(0)
    assert abs(ga.item() - (1.25 ** 2 + 1.0)) < 1e-15
    # dL/dw: g <- g - h a y with (a, y) at the step's start: y = 3.125, a = 1, then y = 3.125 / 1.25 = 2.5 (euler backwards:
    # y - h w y reversed is y (1 - 0.25)), a = 1.25
    y1 = 3.125 * 0.75
    assert abs(gw.item() - (0.5 * 1.0 * 3.125 + 0.5 * 1.25 * y1)) < 1e-15


# ---- validation codes through the ABI ------------------------------------------------------------------------------------------
def gcn_structs(n=8, d=16, groups=16):
    f = _lib.GcnOdeFunc()
    f.n, f.d, f.groups, f.eps = n, d, groups, 1e-5
    return f, _lib.Rk4Workspace()


@pytest.mark.parametrize("method", [EULER, MIDPOINT])
def test_gcn_forward_validation(method):
    fwd = _lib.load().gode_gcn_ode_fixed_forward
    f, ws = gcn_structs()
    res = ctypes.c_void_p()
    ok = lambda m=method, n=4, ff=f: [m, ctypes.byref(ff), DUMMY, ctypes.byref(res), ctypes.byref(ws), 0.0, 1.0, n, None]   # noqa: E731
    for i in (1, 2, 3, 4):
        a = ok()
        a[i] = None
        assert fwd(*a) == E_NULLPTR, i
    assert fwd(*ok(m=-1)) == E_SHAPE and fwd(*ok(m=3)) == E_SHAPE
    a = ok(m=3)
    a[2] = None
    assert fwd(*a) == E_NULLPTR                                        # null pointers come first
    assert fwd(*ok(n=0)) == E_SHAPE and fwd(*ok(n=-2)) == E_SHAPE
    assert fwd(*ok(ff=gcn_structs(n=0)[0])) == E_SHAPE
    assert fwd(*ok()) == E_NULLPTR                                     # ws->S
    assert fwd(*ok(m=0)) == E_NULLPTR                                  # rk4 through the same door: its own ws check


@pytest.mark.parametrize("method", [EULER, MIDPOINT])
def test_gcn_adjoint_validation(method):
    adj = _lib.load().gode_gcn_ode_fixed_adjoint
    yr, ar = ctypes.c_void_p(), ctypes.c_void_p()

    def ok(m=method, n=4, ff=None, ws=None):
        ff = gcn_structs()[0] if ff is None else ff
        ws = gcn_structs()[1] if ws is None else ws
        return [m, ctypes.byref(ff), DUMMY, DUMMY, DUMMY, ctypes.byref(yr), ctypes.byref(ar), ctypes.byref(ws), 0.0, 1.0, n, None]
    for i in (1, 2, 3, 4, 5, 6, 7):
        a = ok()
        a[i] = None
        assert adj(*a) == E_NULLPTR, i
    assert adj(*ok(m=-1)) == E_SHAPE and adj(*ok(m=3)) == E_SHAPE
    assert adj(*ok(n=0)) == E_SHAPE
    assert adj(*ok()) == E_UNSUPPORTED                                 # no small_part: not the launch-bound route
    ws = _lib.Rk4Workspace()
    ws.small_part = 256
    assert adj(*ok(ws=ws)) == E_NULLPTR                                # on the route: the stage buffers are missing
    assert adj(*ok(ws=ws, ff=gcn_structs(n=65537)[0])) == E_UNSUPPORTED            # above the one-launch kernels' rows
    assert adj(*ok(ws=ws, ff=gcn_structs(d=128, groups=32)[0])) == E_UNSUPPORTED   # and beside their widths


@pytest.mark.parametrize("method", [EULER, MIDPOINT])
def test_gcn_forward_save_and_backprop_validation(method):
    lib = _lib.load()
    f, ws = gcn_structs()
    fwd = lib.gode_gcn_ode_fixed_forward_save
    ok = lambda m=method, st=(4, 0, 4), ff=f: [m, ctypes.byref(ff), DUMMY, DUMMY, DUMMY, ctypes.byref(ws), 0.0, 1.0, st[0], st[1], st[2], None]   # noqa: E731
    for i in (1, 2, 3, 4, 5):
        a = ok()
        a[i] = None
        assert fwd(*a) == E_NULLPTR, i
    assert fwd(*ok(m=-1)) == E_SHAPE and fwd(*ok(m=3)) == E_SHAPE
    assert fwd(*ok(st=(0, 0, 1))) == E_SHAPE                           # no steps
    assert fwd(*ok(st=(4, 2, 2))) == E_SHAPE                           # empty range
    assert fwd(*ok(st=(4, 3, 1))) == E_SHAPE                           # out of order
    assert fwd(*ok(st=(4, 0, 5))) == E_SHAPE                           # past the grid
    assert fwd(*ok(ff=gcn_structs(n=0)[0])) == E_SHAPE
    assert fwd(*ok()) == E_NULLPTR                                     # ws->S
    bp = lib.gode_gcn_ode_fixed_backprop
    res = ctypes.c_void_p()
    ws2 = _lib.Rk4Workspace()
    okb = lambda m=method, st=(4, 0, 4): [m, ctypes.byref(f), DUMMY, DUMMY, DUMMY, ctypes.byref(res), ctypes.byref(ws2), None, 0.0, 1.0, st[0], st[1], st[2], None]   # noqa: E731
    for i in (1, 2, 3, 4, 5, 6):
        a = okb()
        a[i] = None
        assert bp(*a) == E_NULLPTR, i
    assert bp(*okb(m=-1)) == E_SHAPE and bp(*okb(m=3)) == E_SHAPE
    assert bp(*okb(st=(0, 0, 1))) == E_SHAPE
    assert bp(*okb(st=(4, 3, 1))) == E_SHAPE
    assert bp(*okb()) == E_NULLPTR                                     # the stage buffers
    for i in range(4):
        ws2.ka[i] = ws2.ktheta[i] = 256
    ws2.dZ = ws2.dS = 256
    assert bp(*okb()) == E_NULLPTR                                     # the partial buffers still missing


def test_small_finish_step_validation():
    fin = _lib.load().gode_gcn_small_finish_step_f32
    f, _ = gcn_structs()
    wb, ts = (ctypes.c_float * 4)(0.5, 0.5, 0.0, 0.0), (ctypes.c_float * 4)()
    assert fin(None, DUMMY, 2, DUMMY, wb, ts, None) == E_NULLPTR
    assert fin(ctypes.byref(f), DUMMY, 2, None, wb, ts, None) == E_NULLPTR
    assert fin(ctypes.byref(f), DUMMY, 0, DUMMY, wb, ts, None) == E_SHAPE
    assert fin(ctypes.byref(f), DUMMY, 5, DUMMY, wb, ts, None) == E_SHAPE
    zero = (ctypes.c_float * 4)()
    assert fin(ctypes.byref(f), DUMMY, 2, DUMMY, zero, ts, None) == E_SHAPE        # every weight zero: nothing to add


def _buf(n=64):
    return (ctypes.c_float * n)()


def gat_structs(n=37, d=16, heads=1, small_part=True):
    """A gode_gat_odefunc_t / gode_gat_workspace_t pair with every pointer the sweeps want set (to host memory)."""
    keep = [_buf() for _ in range(8)]
    a = P(keep[0])
    fs, ws = _lib.GatOdeFunc(), _lib.GatWorkspace()
    for g in (fs.mt, fs.ms_inc, fs.mt_inc):
        g.rowptr = a
    fs.src, fs.tgt, fs.n_edges = a, a, 600
    fs.n, fs.d, fs.groups, fs.eps_gn, fs.eps, fs.heads = n, d, min(32, d) if d > 0 else 1, 1e-5, 1e-6, heads
    for name in ("Wsrc", "Wtgt", "Wlog", "bf", "bw", "gamma", "beta"):
        setattr(fs, name, a)
    for name in ("X", "Ps", "Pt", "A2", "a", "amax", "wgt", "den", "logits_scratch", "dz", "da", "dPs", "dPt", "dA2", "pair", "gp",
                 "bp", "maxpath_scratch", "colsum_scratch", "colsum_scratch2", "zeros", "heads_scratch"):
        setattr(ws, name, a)
    for j in range(3):
        ws.wp[j] = a
    ws.small_part = a if small_part else None
    return fs, ws, keep


@pytest.mark.parametrize("method", [EULER, MIDPOINT])
def test_gat_pair_validation(method):
    lib = _lib.load()
    b = [_buf() for _ in range(8)]
    fs, ws, _keep = gat_structs()
    fwd = lib.gode_gat_ode_fixed_forward_save

    def okf(m=method, st=(4, 0, 4), f=fs, w=ws):
        return [m, ctypes.byref(f), P(b[0]), P(b[1]), P(b[2]), ctypes.byref(w), 0.0, 1.0, st[0], st[1], st[2], None]
    for i in (1, 2, 3, 4, 5):
        a = okf()
        a[i] = None
        assert fwd(*a) == E_NULLPTR, i
    assert fwd(*okf(m=-1)) == E_SHAPE and fwd(*okf(m=3)) == E_SHAPE
    assert fwd(*okf(st=(0, 0, 1))) == E_SHAPE
    assert fwd(*okf(st=(4, 3, 1))) == E_SHAPE
    assert fwd(*okf(st=(4, 0, 5))) == E_SHAPE
    f128, w128, _k = gat_structs(d=128)
    assert fwd(*okf(f=f128, w=w128)) == E_UNSUPPORTED
    fn, wn, _k2 = gat_structs(small_part=False)
    assert fwd(*okf(f=fn, w=wn)) == E_UNSUPPORTED
    bp = lib.gode_gat_ode_fixed_backprop
    S = R.STAGES["euler" if method == EULER else "midpoint"]

    def okb(m=method, st=(4, 0, 4), f=fs, w=ws, ybar=None, a=None, ks=None):
        yb = (ctypes.c_void_p * 4)(*(ybar if ybar is not None else [P(b[3 + s]) for s in range(4)]))
        return [m, ctypes.byref(f), P(b[0]), a or P(b[1]), P(b[2]), yb, ks or P(b[7]), P(b[0]), ctypes.byref(w), 0.0, 1.0,
                st[0], st[1], st[2], None]
    for i in (1, 2, 3, 4, 5, 6, 7, 8):
        a = okb()
        a[i] = None
        assert bp(*a) == E_NULLPTR, i
    assert bp(*okb(m=-1)) == E_SHAPE and bp(*okb(m=3)) == E_SHAPE
    assert bp(*okb(ybar=[None] * 4)) == E_NULLPTR
    assert bp(*okb(st=(0, 0, 1))) == E_SHAPE
    assert bp(*okb(st=(4, 3, 1))) == E_SHAPE
    # aliasing: a Ybar that is the cotangent or the re-evaluated stage, two Ybar that are one array, k_scratch = a
    assert bp(*okb(ybar=[P(b[1])] + [P(b[4 + s]) for s in range(3)])) == E_SHAPE
    assert bp(*okb(ybar=[P(b[7])] + [P(b[4 + s]) for s in range(3)])) == E_SHAPE
    assert bp(*okb(ks=P(b[1]))) == E_SHAPE
    if S > 1:
        assert bp(*okb(ybar=[P(b[3]), P(b[3]), P(b[5]), P(b[6])])) == E_SHAPE
    assert bp(*okb(f=f128, w=w128)) == E_UNSUPPORTED
    assert bp(*okb(f=fn, w=wn)) == E_UNSUPPORTED


# ---- the names ----------------------------------------------------------------------------------------------------------------
def test_method_names():
    from graph_odenet_amd import odeint as OI
    assert OI._method(None) == "dopri5"
    for m in ("dopri5", "rk4", "euler", "midpoint"):
        assert OI._method(m) == m
    for m in ("adams", "tsit5", "Euler", ""):
        with pytest.raises(ValueError, match="dopri5, rk4, euler, midpoint"):
            OI._method(m)


def test_clis_accept_the_new_methods():
    from graph_odenet_amd import train_layers, train_res
    for mod in (train_res, train_layers):
        for m in ("euler", "midpoint", "rk4", "dopri5"):
            a = mod.build_parser().parse_args(["--method", m, "--step_size", "0.0625"])
            assert a.method == m and a.step_size == 0.0625
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--method", "adams"])


def test_fields_offer_the_protocol_members():
    from graph_odenet_amd import gat_ode, gcn_ode, qc_ode, solver
    for name in ("fixed_native", "fixed_forward_save", "fixed_backprop"):
        assert getattr(solver.Field, name) is None
    assert callable(gcn_ode.GcnOdeField.fixed_native) and callable(gcn_ode.GcnOdeAdjointField.fixed_native)
    assert callable(gcn_ode.GcnOdeField.fixed_forward_save) and callable(gcn_ode.GcnOdeField.fixed_backprop)
    assert gcn_ode.GcnOdePartField.fixed_native is None and gcn_ode.GcnOdePartField.fixed_forward_save is None
    assert callable(gat_ode.GatOdeField._fixed_forward_save) and callable(qc_ode.EdgeOdeField._fixed_backprop)
