"""The tableau-driven GAT step drivers and the closing launch of their adjoint step (csrc/gat_small.hip:
gode_gat_small_finish_multi_f32; csrc/gat_driver.hip: gode_gat_ode_adaptive_step_forward / _adjoint / _backprop): they exist,
are bound from the header and return their validation codes in the stated order before any HIP call (no GPU needed); and
the algebra of the edge-conditioned field's tableau-driven sweep (qc_ode.EdgeOdeField._adaptive_step_backprop) on a float64
toy stage against autograd through the step."""
import ctypes

import pytest
import torch

from graph_odenet_amd import _lib
from test_gat_backprop_abi import NULLPTR, SHAPE, UNSUPPORTED, P, _buf, _ptr_array, _structs

NAMES = {"gode_gat_small_finish_multi_f32": 9, "gode_gat_ode_adaptive_step_forward": 13,
         "gode_gat_ode_adaptive_step_adjoint": 23, "gode_gat_ode_adaptive_step_backprop": 19}
STAGES = {0: 7, 1: 4, 2: 3}


def test_symbols_exist_and_are_bound_from_the_header():
    lib = _lib.load()
    for name, nargs in NAMES.items():
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == nargs, name
    assert len(_lib.STRUCTS) == 11                                   # the kernel-argument structs stay internal
    assert [_lib.CONSTANTS["GODE_RKA_" + k] for k in ("DOPRI5", "BOSH3", "ADAPTIVE_HEUN")] == [0, 1, 2]
    # the dopri5 entry points keep their signatures
    assert len(lib.gode_gat_ode_dopri5_step_forward.argtypes) == 12
    assert len(lib.gode_gat_ode_dopri5_step_adjoint.argtypes) == 21
    assert len(lib.gode_gat_ode_dopri5_step_backprop.argtypes) == 18


def test_finish_multi_validation_codes():
    f = _lib.load().gode_gat_small_finish_multi_f32
    b = [_buf() for _ in range(15)]
    ts = (ctypes.c_float * 7)()

    def args(n=37, d=16, heads=1, q=4, kth=None, kat=None):
        return [P(b[0]), n, d, heads, q, _ptr_array(b[1:8] if kth is None else kth), _ptr_array(b[8:15] if kat is None else kat),
                ts, None]
    for i in (0, 5, 6, 7):
        a = args()
        a[i] = None
        assert f(*a) == NULLPTR, i
    a = args(q=0)
    a[0] = None
    assert f(*a) == NULLPTR                                          # null pointers come first
    for q in (0, 8, -1):
        assert f(*args(q=q)) == SHAPE, q
        assert f(*args(q=q, d=128)) == SHAPE, q                       # ... and n_stages before the shape's support
    assert f(*args(n=0)) == SHAPE and f(*args(d=0)) == SHAPE
    assert f(*args(kth=b[1:3] + [None] + b[4:8])) == NULLPTR          # an output of a stage in 0..n_stages-1 is missing
    assert f(*args(kat=b[8:11] + [None] + b[12:15])) == NULLPTR
    for kw in (dict(d=128), dict(d=24), dict(n=65537), dict(d=64, heads=9), dict(d=64, heads=3)):
        assert f(*args(**kw)) == UNSUPPORTED, kw


def _fwd_args(m, fs, ws, k, b):
    return [m, ctypes.byref(fs), P(b[0]), _ptr_array(k), P(b[1]), ctypes.byref(ws), 0.25, 0.125, 1e-3, 1e-3, P(b[2]), P(b[3]), None]


@pytest.mark.parametrize("method", [0, 1, 2])
def test_step_forward_validation_codes(method):
    f = _lib.load().gode_gat_ode_adaptive_step_forward
    S = STAGES[method]
    b = [_buf() for _ in range(4)]
    k = [_buf() for _ in range(S)]
    fs, ws, _k = _structs()
    for i in (1, 2, 3, 4, 5, 10, 11):
        a = _fwd_args(method, fs, ws, k, b)
        a[i] = None
        assert f(*a) == NULLPTR, i
    assert f(*_fwd_args(-1, fs, ws, k, b)) == SHAPE and f(*_fwd_args(3, fs, ws, k, b)) == SHAPE
    a = _fwd_args(3, fs, ws, k, b)
    a[2] = None
    assert f(*a) == NULLPTR                                          # null pointers come before the method
    fs1, ws1, _k1 = _structs()
    fs1.Wlog = None
    assert f(*_fwd_args(3, fs1, ws1, k, b)) == SHAPE                  # the method before the struct's own checks
    assert f(*_fwd_args(method, fs1, ws1, k, b)) == NULLPTR
    fs2, ws2, _k2 = _structs(n=0)
    assert f(*_fwd_args(method, fs2, ws2, k, b)) == SHAPE
    fs3, ws3, _k3 = _structs()
    fs3.act = 99
    assert f(*_fwd_args(method, fs3, ws3, k, b)) == SHAPE             # a message activation outside the list
    assert f(*_fwd_args(method, fs, ws, k[:S - 1] + [None], b)) == NULLPTR      # a stage buffer is missing


def _adj_args(m, fs, ws, ks, b, parts=True):
    return [m, ctypes.byref(fs), P(b[0]), P(b[1]), P(b[2]), P(b[3]), _ptr_array(ks[0]), _ptr_array(ks[1]), _ptr_array(ks[2]),
            _ptr_array(ks[3]), P(b[4]), P(b[5]), P(b[6]), P(b[7]), ctypes.byref(ws), P(b[8]) if parts else None, 1.0, -0.125,
            1e-3, 1e-3, P(b[9]), P(b[10]), None]


@pytest.mark.parametrize("method", [0, 1, 2])
def test_step_adjoint_validation_codes(method):
    f = _lib.load().gode_gat_ode_adaptive_step_adjoint
    S = STAGES[method]
    b = [_buf() for _ in range(11)]
    ks = [[_buf() for _ in range(S)] for _ in range(4)]
    fs, ws, _k = _structs(d=32, heads=4)
    for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 20, 21):
        a = _adj_args(method, fs, ws, ks, b)
        a[i] = None
        assert f(*a) == NULLPTR, i
    for parts in (True, False):                                       # parts is nullable: it is not among the null checks
        assert f(*_adj_args(-1, fs, ws, ks, b, parts)) == SHAPE and f(*_adj_args(3, fs, ws, ks, b, parts)) == SHAPE
    a = _adj_args(3, fs, ws, ks, b)
    a[5] = None
    assert f(*a) == NULLPTR                                          # null pointers come before the method
    fs1, ws1, _k1 = _structs(d=32, heads=4)
    ws1.dPs = None                                                    # a workspace without the adjoint's arrays
    assert f(*_adj_args(3, fs1, ws1, ks, b)) == SHAPE
    assert f(*_adj_args(method, fs1, ws1, ks, b)) == NULLPTR
    fs2, ws2, _k2 = _structs(d=64, heads=3)
    assert f(*_adj_args(method, fs2, ws2, ks, b)) == SHAPE            # heads do not divide d
    for c in range(4):
        bad = [list(x) for x in ks]
        bad[c][S - 1] = None
        assert f(*_adj_args(method, fs, ws, bad, b)) == NULLPTR, c


def _bp_args(m, fs, ws, b, k, yb, first=0, kbar_last=True, kbar1=True):
    wk = (ctypes.c_double * 7)(*[0.1] * 7)
    return [m, ctypes.byref(fs), P(b[0]), _ptr_array(k), P(b[1]), P(b[2]) if kbar_last else None, 1.0, wk, 0.25, 0.125, first,
            _ptr_array(yb), P(b[3]), P(b[4]) if kbar1 else None, P(b[5]), P(b[6]), P(b[7]), ctypes.byref(ws), None]


@pytest.mark.parametrize("method", [0, 1, 2])
def test_step_backprop_validation_codes(method):
    f = _lib.load().gode_gat_ode_adaptive_step_backprop
    S = STAGES[method]
    b = [_buf() for _ in range(8)]
    k = [_buf() for _ in range(S)]
    yb = [_buf() for _ in range(S)]
    fs, ws, _k = _structs(d=32, heads=4)
    for i in (1, 2, 3, 4, 7, 11, 12, 14, 15, 16, 17):
        a = _bp_args(method, fs, ws, b, k, yb)
        a[i] = None
        assert f(*a) == NULLPTR, i
    assert f(*_bp_args(-1, fs, ws, b, k, yb)) == SHAPE and f(*_bp_args(3, fs, ws, b, k, yb)) == SHAPE
    a = _bp_args(3, fs, ws, b, k, yb)
    a[4] = None
    assert f(*a) == NULLPTR                                          # null pointers come before the method
    assert f(*_bp_args(3, fs, ws, b, k, yb, first=0, kbar1=False)) == NULLPTR       # ... kbar1's, wanted unless first, too
    assert f(*_bp_args(3, fs, ws, b, k, yb, first=1, kbar1=False)) == SHAPE
    fs1, ws1, _k1 = _structs(d=128, heads=8)
    assert f(*_bp_args(3, fs1, ws1, b, k, yb)) == SHAPE               # the method before the route
    assert f(*_bp_args(method, fs1, ws1, b, k, yb)) == UNSUPPORTED
    assert f(*_bp_args(method, fs1, ws1, b, k, [None] + yb[1:], first=0, kbar_last=False)) == UNSUPPORTED
    assert f(*_bp_args(method, fs, ws, b, k, yb, first=0, kbar1=False)) == NULLPTR            # kbar1 is a result unless first
    assert f(*_bp_args(method, fs, ws, b, k[:S - 1] + [None], yb)) == NULLPTR
    assert f(*_bp_args(method, fs, ws, b, k, yb[:1] + [None] + yb[2:])) == NULLPTR
    assert f(*_bp_args(method, fs, ws, b, k, [None] + yb[1:], first=1)) == NULLPTR            # Ybar_1 is wanted when first
    # the alias checks of the dopri5 form, before the route is looked at
    for fsx, wsx in ((fs, ws), (fs1, ws1)):
        assert f(*_bp_args(method, fsx, wsx, b, k, yb[:1] + [b[1]] + yb[2:])) == SHAPE        # a Ybar is g
        assert f(*_bp_args(method, fsx, wsx, b, k, yb[:1] + [b[2]] + yb[2:])) == SHAPE        # a Ybar is kbar_last
        assert f(*_bp_args(method, fsx, wsx, b, k, yb[:1] + [b[3]] + yb[2:])) == SHAPE        # a Ybar is ybar_n
        assert f(*_bp_args(method, fsx, wsx, b, k, yb[:1] + [b[4]] + yb[2:])) == SHAPE        # a Ybar is kbar1
        assert f(*_bp_args(method, fsx, wsx, b, k, yb[:1] + [b[6]] + yb[2:])) == SHAPE        # a Ybar is k_scratch
        assert f(*_bp_args(method, fsx, wsx, b, k, yb[:1] + [yb[2]] + yb[2:])) == SHAPE       # two Ybar share an array
    a = _bp_args(method, fs, ws, b, k, yb)
    a[12] = P(b[1])
    assert f(*a) == SHAPE                                            # ybar_n is g
    a = _bp_args(method, fs, ws, b, k, yb)
    a[15] = P(b[2])
    assert f(*a) == SHAPE                                            # k_scratch is kbar_last
    a = _bp_args(method, fs, ws, b, k, yb)
    a[13] = P(b[3])
    assert f(*a) == SHAPE                                            # kbar1 is ybar_n
    fs2, ws2, _k2 = _structs(d=32, heads=4, small_part=False)
    assert f(*_bp_args(method, fs2, ws2, b, k, yb, first=1, kbar1=False)) == UNSUPPORTED
    fs3, ws3, _k3 = _structs(n=-5, d=32, heads=4)
    assert f(*_bp_args(method, fs3, ws3, b, k, yb)) == SHAPE


def test_members_are_offered_per_instance():
    """The classes keep the protocol's defaults; a field binds the adaptive members where it serves them."""
    import os
    from graph_odenet_amd import gat_ode, qc_ode
    # the GAT fields' adaptive members are an opt-in: off unless the environment asks
    assert gat_ode.GatOdeField.ADAPTIVE_NATIVE == (os.environ.get("GODE_GAT_ADAPTIVE_NATIVE", "0") == "1")
    assert gat_ode.GatOdeAdjointField.ADAPTIVE_NATIVE == gat_ode.GatOdeField.ADAPTIVE_NATIVE
    for cls in (gat_ode.GatOdeField, gat_ode.GatOdeAdjointField, qc_ode.EdgeOdeField):
        for name in ("adaptive_step_native", "adaptive_step_backprop", "adaptive_backprop_work"):
            assert getattr(cls, name) is None, (cls, name)
    for name in ("_adaptive_step_native", "_adaptive_step_backprop", "_adaptive_backprop_work"):
        assert callable(getattr(gat_ode.GatOdeField, name))
    assert gat_ode.GatOdeAdjointField._adaptive_step_native is not gat_ode.GatOdeField._adaptive_step_native
    for name in ("_adaptive_step_backprop", "_adaptive_backprop_work"):
        assert callable(getattr(qc_ode.EdgeOdeField, name))


# ---- the edge-conditioned field's sweep from a tableau: float64 toy stage, no library -------------------------------------------
def _toy_field(W):
    """An EdgeOdeField whose stage is k = tanh(Y W + t) in torch float64: _stage_bwd and _close_step replaced, the sweep's own
    algebra (cotangents, skipped stages, the closing combinations) kept."""
    from graph_odenet_amd import qc_ode
    fld = object.__new__(qc_ode.EdgeOdeField)

    def stage_bwd(q, cot, k, yin, t, ybar):
        c = sum(cf * x for cf, x in cot)
        Y = sum(cf * x for cf, x in yin).detach().requires_grad_(True)
        Wl = W.detach().requires_grad_(True)
        gy, gw = torch.autograd.grad(torch.tanh(Y @ Wl + t), (Y, Wl), c)
        ybar.copy_(gy)
        return gw

    def close_step(stages, theta):
        for gw in stages:
            theta.add_(gw.reshape(-1))
    fld._stage_bwd, fld._close_step = stage_bwd, close_step
    return fld


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("method", ["dopri5", "bosh3", "adaptive_heun"])
def test_edge_field_sweep_algebra_on_a_float64_toy(method, first, monkeypatch):
    """(ybar_n, kbar_1, theta) of one step against autograd of L = <g, wy y + sum wk_s k_s> + <kbar_last, k_S>, k_1 an input of
    its own unless `first` (then k_1 = f(t, y) is part of the graph)."""
    from graph_odenet_amd import ops
    from graph_odenet_amd.solver import ADAPTIVE_TABLEAUS

    def lincomb_(out, terms):
        out.copy_(sum(c * x for c, x in terms))
    monkeypatch.setattr(ops, "lincomb_", lincomb_)
    monkeypatch.setattr(ops, "lincomb_multi_", lambda outs, tl: [lincomb_(o, t) for o, t in zip(outs, tl)])
    C, A, B = ADAPTIVE_TABLEAUS[method][:3]
    S = len(C)
    n, d, t, h = 5, 3, 0.3, 0.2
    gen = torch.Generator().manual_seed(11 + S)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)      # noqa: E731
    W, y, g, kbar_last = 0.5 * rnd(d, d), rnd(n, d), rnd(n, d), rnd(n, d)
    wy = 0.9
    wk = [h * bq * 0.8 + (0.01 if q == S - 1 else 0.0) for q, bq in enumerate(B)]     # a weight on k_S too, b_2 = 0 under dopri5 kept
    f = lambda tt, Y, Wl: torch.tanh(Y @ Wl + tt)                             # noqa: E731
    yv, Wv = y.clone().requires_grad_(True), W.clone().requires_grad_(True)
    k1 = f(t, yv, Wv) if first else f(t, y, W).detach().requires_grad_(True)
    ks = [k1]
    for q in range(1, S):
        ks.append(f(t + C[q] * h, yv + h * sum(A[q][j] * ks[j] for j in range(q) if A[q][j] != 0.0), Wv))
    L = (g * (wy * yv + sum(wk[q] * ks[q] for q in range(S)))).sum() + (kbar_last * ks[S - 1]).sum()
    want = torch.autograd.grad(L, (yv, Wv) if first else (yv, Wv, k1))
    fld = _toy_field(W)
    work = fld._adaptive_backprop_work(method, y)
    assert len(work["ybar"]) == S and len(work["pairs"]) == 2
    theta = torch.zeros(d * d, dtype=torch.float64)
    ybar_n, kbar1 = fld._adaptive_step_backprop(method, y, [k.detach() for k in ks], g, kbar_last, wy, wk, t, h, first, work, 1, theta)
    assert ybar_n is work["pairs"][1][0]
    assert torch.allclose(ybar_n, want[0], rtol=1e-12, atol=1e-13)
    assert torch.allclose(theta.view(d, d), want[1], rtol=1e-12, atol=1e-13)
    if first:
        assert kbar1 is None
    else:
        assert kbar1 is work["pairs"][1][1] and torch.allclose(kbar1, want[2], rtol=1e-12, atol=1e-13)
    if method == "dopri5":
        # the dopri5 member is the general one under the dopri5 tableau
        theta2 = torch.zeros_like(theta)
        work2 = fld._dopri5_backprop_work(y)
        yb2, kb2 = fld._dopri5_step_backprop(y, [k.detach() for k in ks], g, kbar_last, wy, wk, t, h, first, work2, 0, theta2)
        assert len(work2["ybar"]) == 7 and torch.equal(yb2, ybar_n) and torch.equal(theta2, theta)
        assert (kb2 is None) if first else torch.equal(kb2, kbar1)
