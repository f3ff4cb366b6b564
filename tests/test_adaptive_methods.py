"""The adaptive methods bosh3 and adaptive_heun without a GPU: the algebra of their tableaus, the tables of solver.py against
the restatement's (tests/adaptive_methods_ref.py) and the C drivers' (gode_rka_*), the orders of the float64 restatement the
GPU tests compare against, the validation codes of the new entry points and of the fused step close (they come back before
any HIP call; pointers that must never be dereferenced are dummies), and the names odeint and the two CLIs accept."""
import ctypes
import math

import pytest
import torch

import adaptive_methods_ref as R
from graph_odenet_amd import _lib

E_NULLPTR, E_SHAPE = -1, -2
DUMMY = ctypes.c_void_p(256)          # a non-NULL device address the validation never touches
NEW = ["bosh3", "adaptive_heun"]
P = ctypes.addressof


# ---- tableaus ---------------------------------------------------------------------------------------------------------------
def tables(source, name):
    """(c, a, b, e, p) of a method as the product (solver.ADAPTIVE_TABLEAUS) or the restatement states it."""
    if source == "restatement":
        return R.TABLEAUS[name]
    from graph_odenet_amd import solver
    c, a, b, e, p = solver.ADAPTIVE_TABLEAUS[name]
    return list(c), [list(r) for r in a], list(b), list(e), p


@pytest.mark.parametrize("source", ["product", "restatement"])
@pytest.mark.parametrize("name", ["dopri5"] + NEW)
def test_tableau_algebra(name, source):
    c, a, b, e, p = tables(source, name)
    S = len(c)
    bs = [bi - ei for bi, ei in zip(b, e)]                         # the embedded solution's weights
    assert len(a) == S and len(b) == S and len(e) == S and all(len(a[s]) == s for s in range(S))
    assert abs(sum(b) - 1.0) < 1e-15 and abs(sum(e)) < 1e-15
    for s in range(S):
        assert abs(c[s] - sum(a[s])) < 1e-15, (name, s)
    assert list(a[S - 1]) == list(b[:S - 1]) and b[S - 1] == 0       # FSAL form: the last row of a is b
    full = [list(a[s]) + [0.0] * (S - s) for s in range(S)]

    def conditions(w, order):
        out = []
        if order >= 1:
            out.append((sum(w), 1.0))
        if order >= 2:
            out.append((sum(wi * ci for wi, ci in zip(w, c)), 1 / 2))
        if order >= 3:
            out.append((sum(wi * ci * ci for wi, ci in zip(w, c)), 1 / 3))
            out.append((sum(w[i] * full[i][j] * c[j] for i in range(S) for j in range(S)), 1 / 6))
        return out
    for got, want in conditions(b, min(p, 3)) + conditions(bs, min(p - 1, 3)):
        assert abs(got - want) < 1e-14, (name, got, want)


def test_python_tables_are_the_restatements_and_the_c_drivers():
    from graph_odenet_amd import solver
    lib = _lib.load()
    assert [_lib.CONSTANTS["GODE_RKA_" + k] for k in ("DOPRI5", "BOSH3", "ADAPTIVE_HEUN")] == [0, 1, 2]
    assert solver.ADAPTIVE_METHODS == ("dopri5", "bosh3", "adaptive_heun")
    for code, name in enumerate(solver.ADAPTIVE_METHODS):
        c, a, b, e, p = solver.ADAPTIVE_TABLEAUS[name]
        S = len(c)
        assert solver.adaptive_code(name) == code == R.CODES[name] and solver.adaptive_stages(name) == S == R.STAGES[name]
        rc, ra, rb, re_, rp = R.TABLEAUS[name]
        assert (list(c), [list(r) for r in a], list(b), p) == (rc, [list(r) for r in ra], rb, rp), name
        assert max(abs(u - v) for u, v in zip(e, re_)) < 1e-17, name
        assert lib.gode_rka_stages(code) == S and lib.gode_rka_order(code) == p
        cc, bb, ee = ((ctypes.c_double * S)() for _ in range(3))
        aa = (ctypes.c_double * (S * S))()
        assert lib.gode_rka_tableau(code, cc, aa, bb, ee) == 0
        assert list(cc) == list(c) and list(bb) == list(b) and list(ee) == list(e)
        for s in range(S):
            assert list(aa[s * S:(s + 1) * S]) == list(a[s]) + [0.0] * (S - len(a[s])), (name, s)
        assert lib.gode_rka_tableau(code, None, None, None, None) == 0
        for x in (0.0, 0.3, 1.0):
            got, want = solver.adaptive_interp_weights(name, x), R.interp_weights(name, x)
            assert got[0] == want[0] and got[1] == want[1] and list(got[2]) == list(want[2])
    for bad in (-1, 3):
        assert lib.gode_rka_stages(bad) == E_SHAPE and lib.gode_rka_order(bad) == E_SHAPE
        assert lib.gode_rka_tableau(bad, None, None, None, None) == E_SHAPE
    assert lib.gode_rk_stages(3) == E_SHAPE                          # the fixed-grid codes are a namespace of their own


@pytest.mark.parametrize("source", ["product", "restatement"])
@pytest.mark.parametrize("method,lo,hi", [("bosh3", 7.0, 9.0), ("adaptive_heun", 3.6, 4.5)])
def test_tables_have_the_order_they_should(method, lo, hi, source, monkeypatch):
    """y' = -y over [0, 1] in float64 with forced equal steps, n = 8 then 16, the restatement's loop over the product's tables
    and over its own: the error ratio is 2^p up to the next term."""
    monkeypatch.setitem(R.TABLEAUS, method, tables(source, method))
    y0 = torch.ones(3, dtype=torch.float64)
    errs = []
    for n in (8, 16):
        y, seq, nfe = R.solve(lambda t, y: -y, y0, 0.0, 1.0, method, 1e-3, 1e-3, forced=[(1.0 / n, True)] * n)
        assert len(seq) == n and nfe == 2 + (R.STAGES[method] - 1) * n
        errs.append((y - math.exp(-1.0)).abs().max().item())
    ratio = errs[0] / errs[1]
    print("%s: errors %.6e %.6e ratio %.4f" % (method, errs[0], errs[1], ratio))
    assert lo <= ratio <= hi


@pytest.mark.parametrize("method", NEW)
def test_hermite_fit_at_the_middle_of_a_step(method):
    """The fit itself on y' = -y: the cubic through (y_n, f_n, y_{n+1}, f_{n+1}) of one step of size 1/8 from t = 0, at x =
    1/2, is within 1e-6 of exp(-1/16) (its own error is h^4 / 384 = 6.4e-7; the end values are the exact ones - a step's own
    y_{n+1} carries the method's local error, 1e-5 for bosh3 at this h, which is not the fit's).  The restatement's solve
    applies the same weights: a forced step cut at t = 1/16 returns that combination of ITS y_{n+1} and stages."""
    from graph_odenet_amd import solver
    h, S = 1.0 / 8, R.STAGES[method]
    for weights in (R.interp_weights(method, 0.5), solver.adaptive_interp_weights(method, 0.5)):
        cy0, cy1, kc = weights
        assert all(kc[s] == 0.0 for s in range(1, S - 1))
        got = cy0 * 1.0 + cy1 * math.exp(-h) + h * (kc[0] * -1.0 + kc[S - 1] * -math.exp(-h))
        print("%s: hermite error %.3e" % (method, abs(got - math.exp(-h / 2))))
        assert abs(got - math.exp(-h / 2)) < 1e-6
    y0 = torch.ones(1, dtype=torch.float64)
    c, a, b = R.TABLEAUS[method][:3]
    y, seq, _ = R.solve(lambda t, y: -y, y0, 0.0, 1.0 / 16, method, 1e-3, 1e-3, forced=[(h, True)])
    ks = []
    for s in range(S):
        ks.append(-(1.0 + h * sum(a[s][j] * ks[j] for j in range(s))))
    y1 = 1.0 + h * sum(b[s] * ks[s] for s in range(S))
    assert len(seq) == 1 and abs(y.item() - (cy0 + cy1 * y1 + h * (kc[0] * ks[0] + kc[S - 1] * ks[S - 1]))) < 1e-15
    cy0, cy1, kc = R.interp_weights(method, 1.0)
    assert (cy0, cy1) == (0.0, 1.0) and all(v == 0.0 for v in kc)


def test_restatement_controller_rejects_and_recovers():
    """A stiff-ish linear field at a loose first step: the free-running controller rejects at least once, every accepted
    ratio is <= 1, and the result is within the tolerance's reach of the exact one."""
    y0 = torch.ones(4, dtype=torch.float64)
    y, seq, nfe = R.solve(lambda t, y: -30.0 * y * (1 + t), y0, 0.0, 1.0, "bosh3", 1e-5, 1e-5)
    assert any(not acc for _, acc, _ in seq) and all(r <= 1.0 for _, acc, r in seq if acc)
    assert nfe == 2 + 3 * len(seq)
    assert abs(y[0].item() - math.exp(-45.0)) < 1e-4
    # the product's controller proposes the same next step after every attempt of that run, growth and shrinkage alike
    from graph_odenet_amd import solver
    for (dt, _, ratio), (dt_next, _, _) in zip(seq, seq[1:]):
        assert abs(solver._optimal_step(dt, ratio, order=3) - dt_next) <= 1e-15 * dt_next


@pytest.mark.parametrize("name", ["dopri5"] + NEW)
def test_product_controller_is_the_restatements(name):
    """solver._optimal_step with the method's order against the restatement's optimal_step: no error, accepted, rejected, and
    both clamps (growth 10, shrink 0.2); and the exponent really is 1/p - another order gives another step."""
    from graph_odenet_amd import solver
    p = solver.ADAPTIVE_TABLEAUS[name][4]
    assert p == R.TABLEAUS[name][4] == {"dopri5": 5, "bosh3": 3, "adaptive_heun": 2}[name]
    for dt in (1e-3, 0.37):
        for ratio in (0.0, 1e-12, 0.04, 0.5, 1.0, 1.7, 40.0, 1e9):
            got, want = solver._optimal_step(dt, ratio, order=p), R.optimal_step(dt, ratio, p)
            assert abs(got - want) <= 1e-15 * want, (dt, ratio)
        assert solver._optimal_step(dt, 0.04, order=p) != solver._optimal_step(dt, 0.04, order=p + 1)
        assert solver._optimal_step(dt, 1e9, order=p) == 0.2 * dt and solver._optimal_step(dt, 0.0, order=p) == 10.0 * dt


# ---- validation codes through the ABI ------------------------------------------------------------------------------------------
def gcn_structs(n=8, d=16, groups=16):
    f = _lib.GcnOdeFunc()
    f.n, f.d, f.groups, f.eps = n, d, groups, 1e-5
    return f, _lib.Rk4Workspace()


def _ptrs(S, fill=256):
    return (ctypes.c_void_p * 7)(*([fill] * S + [None] * (7 - S)))


@pytest.mark.parametrize("method", [0, 1, 2])
def test_step_forward_validation(method):
    fwd = _lib.load().gode_gcn_ode_adaptive_step_forward
    f, ws = gcn_structs()
    S = _lib.load().gode_rka_stages(method)
    ok = lambda m=method, ff=f, k=None: [m, ctypes.byref(ff), DUMMY, k or _ptrs(S), DUMMY, ctypes.byref(ws), 0.0, 0.1, 1e-3,   # noqa: E731
                                         1e-3, DUMMY, DUMMY, None]
    for i in (1, 2, 3, 4, 5, 10, 11):
        a = ok()
        a[i] = None
        assert fwd(*a) == E_NULLPTR, i
    assert fwd(*ok(m=-1)) == E_SHAPE and fwd(*ok(m=3)) == E_SHAPE
    a = ok(m=3)
    a[2] = None
    assert fwd(*a) == E_NULLPTR                                        # null pointers come first
    assert fwd(*ok(ff=gcn_structs(n=0)[0])) == E_SHAPE
    assert fwd(*ok(k=_ptrs(S - 1))) == E_NULLPTR                       # a stage buffer is missing
    assert fwd(*ok()) == E_NULLPTR                                     # ws->S


@pytest.mark.parametrize("method", [0, 1, 2])
def test_step_adjoint_validation(method):
    adj = _lib.load().gode_gcn_ode_adaptive_step_adjoint
    f, ws = gcn_structs()
    S = _lib.load().gode_rka_stages(method)
    ok = lambda m=method, ff=f, k=None: [m, ctypes.byref(ff), DUMMY, DUMMY, DUMMY, _ptrs(S), k or _ptrs(S), _ptrs(S), DUMMY,   # noqa: E731
                                         DUMMY, DUMMY, ctypes.byref(ws), 1.0, -0.1, 1e-3, 1e-3, DUMMY, DUMMY, None]
    for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17):
        a = ok()
        a[i] = None
        assert adj(*a) == E_NULLPTR, i
    assert adj(*ok(m=-1)) == E_SHAPE and adj(*ok(m=3)) == E_SHAPE
    assert adj(*ok(ff=gcn_structs(d=0)[0])) == E_SHAPE
    assert adj(*ok(k=_ptrs(S - 1))) == E_NULLPTR
    assert adj(*ok()) == E_NULLPTR                                     # the workspace arrays


@pytest.mark.parametrize("method", [0, 1, 2])
def test_step_backprop_validation(method):
    bp = _lib.load().gode_gcn_ode_adaptive_step_backprop
    f, ws = gcn_structs()
    S = _lib.load().gode_rka_stages(method)
    wk = (ctypes.c_double * 7)(*([0.1] * 7))
    b = [(ctypes.c_float * 4)() for _ in range(12)]

    def ok(m=method, ff=f, first=0, ybar=None, ybar_n=None, kbar1=0, g=None):
        yb = (ctypes.c_void_p * 7)(*(ybar if ybar is not None else [P(b[s]) for s in range(S)]))
        return [m, ctypes.byref(ff), DUMMY, _ptrs(S), g or P(b[8]), P(b[9]), 1.0, wk, 0.0, 0.1, first, yb, ybar_n or P(b[10]),
                P(b[11]) if kbar1 == 0 else kbar1, DUMMY, _ptrs(S), ctypes.byref(ws), None, None]
    for i in (1, 2, 3, 4, 7, 11, 12, 14, 15, 16):
        a = ok()
        a[i] = None
        assert bp(*a) == E_NULLPTR, i
    assert bp(*ok(m=-1)) == E_SHAPE and bp(*ok(m=3)) == E_SHAPE
    assert bp(*ok(ff=gcn_structs(n=-1)[0])) == E_SHAPE
    assert bp(*ok(kbar1=None)) == E_NULLPTR                            # not first: kbar_1 must have a home
    assert bp(*ok(ybar=[P(b[0])] + [None] * (S - 1))) == E_NULLPTR
    assert bp(*ok(first=1, ybar=[None] + [P(b[s]) for s in range(1, S)])) == E_NULLPTR
    # aliasing: the results and the work arrays are never the cotangent g or the arriving kbar
    assert bp(*ok(ybar_n=P(b[8]))) == E_SHAPE and bp(*ok(ybar_n=P(b[9]))) == E_SHAPE
    assert bp(*ok(kbar1=P(b[8]))) == E_SHAPE and bp(*ok(kbar1=P(b[10]))) == E_SHAPE
    assert bp(*ok(ybar=[P(b[0]), P(b[8])] + [P(b[s]) for s in range(2, S)])) == E_SHAPE
    assert bp(*ok(ybar=[P(b[0]), P(b[10])] + [P(b[s]) for s in range(2, S)])) == E_SHAPE
    assert bp(*ok()) == E_NULLPTR                                      # the workspace arrays


def test_close_kernel_validation():
    lib = _lib.load()
    close = lib.gode_rk_close_err_multi_f32
    assert lib.gode_rk_close_err_scratch_bytes() >= 4 * 8
    b = [(ctypes.c_float * 8)() for _ in range(6)]

    def call(count=1, nterms=3, y1=None, n=8, drop=None, ec_null=False, term_null=False):
        lcs = (_lib.LinComb * 4)()
        for c in range(4):
            lcs[c].n = nterms
            for j in range(min(max(nterms, 0), _lib.GODE_MAX_TERMS)):
                lcs[c].coef[j] = 1.0
                lcs[c].ptr[j] = None if (term_null and j == 1) else P(b[j % 4])
        y1s = (ctypes.c_void_p * 4)(*[P(b[4]) if y1 is None else y1] * 4)
        ec = (ctypes.c_float * 8)()
        ecs = (ctypes.c_void_p * 4)(*[None if ec_null else P(ec)] * 4)
        ns = (ctypes.c_int64 * 4)(*[n] * 4)
        args = [y1s, lcs, ecs, ns, count, 1e-3, 1e-3, DUMMY, DUMMY, None]
        if drop is not None:
            args[drop] = None
        return close(*args)
    for i in (0, 1, 2, 3, 7, 8):
        assert call(drop=i) == E_NULLPTR, i
    assert call(ec_null=True) == E_NULLPTR and call(term_null=True) == E_NULLPTR
    assert call(count=0) == E_SHAPE and call(count=5) == E_SHAPE
    assert call(nterms=_lib.GODE_MAX_TERMS + 1) == E_SHAPE and call(nterms=0) == E_SHAPE
    assert call(n=0) == E_SHAPE
    assert call(y1=P(b[0])) == E_SHAPE and call(y1=P(b[2])) == E_SHAPE     # y1 is one of its own terms
    assert call(count=4, y1=P(b[1])) == E_SHAPE


# ---- the names ----------------------------------------------------------------------------------------------------------------
def test_method_names():
    from graph_odenet_amd import odeint as OI
    assert OI.METHODS == ("dopri5", "rk4", "euler", "midpoint", "bosh3", "adaptive_heun")
    assert OI._method(None) == "dopri5"
    for m in OI.METHODS:
        assert OI._method(m) == m
    for m in ("adams", "tsit5", "Bosh3", ""):
        with pytest.raises(ValueError, match="dopri5, rk4, euler, midpoint, bosh3, adaptive_heun"):
            OI._method(m)


def test_clis_accept_the_new_methods():
    from graph_odenet_amd import train_layers, train_res
    for mod in (train_res, train_layers):
        for m in NEW:
            assert mod.build_parser().parse_args(["--method", m]).method == m
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(["--method", "adams"])


def test_fields_offer_the_protocol_members():
    from graph_odenet_amd import gat_ode, gcn_ode, qc_ode, solver
    for name in ("adaptive_step_native", "adaptive_step_backprop", "adaptive_backprop_work"):
        assert getattr(solver.Field, name) is None
        assert callable(getattr(gcn_ode.GcnOdeField, name))
        # the GAT and edge-conditioned fields run these methods on the per-stage driver: their seven-stage step members are
        # dopri5's alone
        assert getattr(gat_ode.GatOdeField, name, None) is None and getattr(qc_ode.EdgeOdeField, name, None) is None
    assert callable(gcn_ode.GcnOdeAdjointField.adaptive_step_native)
    assert gcn_ode.GcnOdePartField.adaptive_step_native is None and gcn_ode.GcnOdePartField.adaptive_step_backprop is None


def test_record_drops_to_k1_past_the_byte_bound_at_any_stage_count():
    from graph_odenet_amd.solver import Dopri5Record
    y = [torch.zeros(10)]
    for S in (3, 4, 7):
        rec = Dopri5Record(S, max_bytes=(1 + S) * 40 + 1, full=S)
        kk = [[torch.zeros(10)] for _ in range(S)]
        assert rec.accepted(0.0, 0.1, None, y, kk) == S
        assert rec.accepted(0.1, 0.1, None, y, kk) == 1 and all(len(s[4]) == 1 for s in rec.steps)
    assert Dopri5Record(7).full == 7
