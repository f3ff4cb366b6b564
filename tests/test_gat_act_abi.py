"""The activation argument of the edge-attention entry points (graphode.h: gode_gat_act_t on gode_gat_agg_f32_fwd / _bwd,
their route twins and gode_gat_agg_heads_f32_fwd), on the CPU: the symbols, signatures and constants, the checks that come
before everything else, the dispatch (it does not
depend on the activation), gat_layers.message_activation, and the teeth of test_gpu_gat_act.py's comparisons.  The route
queries launch nothing and read only the values of the pointers they are given, so the pointers here are made up
(test_gat_routes.py's).
"""
import ctypes
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_routes_design as D                                           # noqa: E402
import test_gat_routes as T                                             # noqa: E402  (made-up pointers, graph(), proj())
import test_gpu_gat_act as A                                            # noqa: E402  (the float64 restatement with activation)

from graph_odenet_amd import _lib                                       # noqa: E402

E_SHAPE, E_UNSUPPORTED = -2, -5
# the entry points that took the activation as `int32_t act, float act_param` before gode_gat_act_t did
GONE = ("gode_gat_agg_act_f32_fwd", "gode_gat_agg_act_f32_fwd_route", "gode_gat_agg_act_f32_bwd", "gode_gat_agg_act_f32_bwd_route",
        "gode_gat_agg_ode_f32_fwd", "gode_gat_agg_ode_f32_fwd_route", "gode_gat_agg_ode_f32_bwd", "gode_gat_agg_ode_f32_bwd_route",
        "gode_gat_agg_heads_ode_f32_fwd")
CODES = {"RELU": 0, "IDENTITY": 1, "LEAKY_RELU": 2, "ELU": 3, "TANH": 4, "SIGMOID": 5}
P, vp = T.P, T.vp


def want_signatures():
    """The five aggregation signatures written out: the plain ones from before the activation argument, with
    POINTER(gode_gat_act_t) before `stream`."""
    c, i64, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    graph, proj, lincomb, act = (ctypes.POINTER(s) for s in (_lib.Graph, _lib.GatProj, _lib.LinComb, _lib.GatAct))
    fwd = [graph, c, c, proj, i64, c, c, c, f32, c, c, c, act, c]
    bwd = [graph, c, c, proj, i64, c, c, c, c, c, lincomb, f32, c, c, c, i64, c, i64, c, act, c]
    heads = [graph, c, c, proj, i64, c, c, c, i64, i64, f32, c, c, c, act, c]
    return {"gode_gat_agg_f32_fwd": fwd, "gode_gat_agg_f32_fwd_route": fwd, "gode_gat_agg_f32_bwd": bwd,
            "gode_gat_agg_f32_bwd_route": bwd, "gode_gat_agg_heads_f32_fwd": heads}


def test_symbols_constants_and_struct_count():
    lib = _lib.load()
    sig = _lib.SIGNATURES
    for name, argtypes in want_signatures().items():
        assert hasattr(lib, name) and sig[name][0] is ctypes.c_int and sig[name][1] == argtypes, name
    for kind in ("fwd", "bwd"):                                          # a route twin takes what its launcher takes
        assert sig["gode_gat_agg_f32_%s_route" % kind] == sig["gode_gat_agg_f32_%s" % kind]
    assert sorted(n for n in sig if n.startswith("gode_gat_agg_")) == sorted(want_signatures())
    for name in GONE:
        assert name not in sig and not hasattr(lib, name), name
    assert _lib.GatAct._fields_ == [("act", ctypes.c_int32), ("act_param", ctypes.c_float), ("outer_relu", ctypes.c_int32)]
    assert ctypes.sizeof(_lib.GatAct) == 12
    fresh = _lib.GatAct()
    assert (fresh.act, fresh.act_param, fresh.outer_relu) == (0, 0.0, 0)  # zeroed: relu messages, no outer relu
    for k, want in CODES.items():
        assert _lib.CONSTANTS["GODE_GAT_ACT_" + k] == want
    assert len(_lib.STRUCTS) == 11
    from graph_odenet_amd import ops
    assert (ops.GAT_ACT_RELU, ops.GAT_ACT_IDENTITY, ops.GAT_ACT_LEAKY_RELU, ops.GAT_ACT_ELU, ops.GAT_ACT_TANH,
            ops.GAT_ACT_SIGMOID) == (0, 1, 2, 3, 4, 5)


# ---- the activation without the outer relu, on test_gat_routes.py's made-up arguments -------------------------------------
def fwd_act(act, param, n_rows, o, out=0, g=None, launch=False):
    return T.fwd(n_rows, o, out=out, g=g, act=_lib.GatAct(act, param, 0), launch=launch)


def bwd_act(act, param, n_rows, o, terms=0, out=0, g=None, launch=False):
    # T.bwd asserts that the flag is untouched: neither a query nor a refused call writes it
    return T.bwd(n_rows, o, terms, out=out, g=g, act=_lib.GatAct(act, param, 0), launch=launch)


def test_the_new_checks_come_first():
    nan, inf = float("nan"), float("inf")
    for launch in (False, True):                                         # the launching calls answer the same before any launch
        for act in (-1, 6, 1 << 20):
            assert fwd_act(act, 0.0, 700, 16, launch=launch) == E_SHAPE and bwd_act(act, 0.0, 700, 16, launch=launch) == E_SHAPE
        for act in (CODES["LEAKY_RELU"], CODES["ELU"]):
            for bad in (nan, inf, -inf):
                assert fwd_act(act, bad, 700, 16, launch=launch) == E_SHAPE and bwd_act(act, bad, 700, 16, launch=launch) == E_SHAPE
        for act in (1, 2, 3, 4, 5):
            assert bwd_act(act, 0.5, 700, 16, terms=3, launch=launch) == E_UNSUPPORTED
    # before any pointer is looked at: with nothing but NULLs the old entry answers NULLPTR, the new check answers first
    lib = _lib.load()
    nulls_f = (None, None, None, None, 16, None, None, None, 0.0, None, None, None)
    nulls_b = (None, None, None, None, 16, None, None, None, None, None, None, 1.0, None, None, None, 16, None, 2, None)
    act = lambda code, param: ctypes.byref(_lib.GatAct(code, param, 0))  # noqa: E731
    for fn, nulls in ((lib.gode_gat_agg_f32_fwd, nulls_f), (lib.gode_gat_agg_f32_fwd_route, nulls_f),
                      (lib.gode_gat_agg_f32_bwd, nulls_b), (lib.gode_gat_agg_f32_bwd_route, nulls_b)):
        assert fn(*nulls, act(6, 0.0), None) == E_SHAPE and fn(*nulls, act(CODES["ELU"], nan), None) == E_SHAPE
        assert fn(*nulls, act(CODES["ELU"], 1.0), None) == T.E_NULLPTR   # then the old entry's checks, with its codes
    # a parameter nobody reads may be anything; relu with cot terms is the old entry's route
    assert fwd_act(CODES["TANH"], nan, 700, 16) == T.code(T.PF, 4) and fwd_act(CODES["RELU"], nan, 700, 16) == T.code(T.PF, 4)
    for n_rows in (T.BELOW, T.ABOVE):
        for o in (16, 24):
            assert bwd_act(CODES["RELU"], 0.0, n_rows, o, terms=3) == T.bwd(n_rows, o, 3) > 0
    # the old entry's validation codes come back unchanged
    for act in CODES.values():
        assert fwd_act(act, 0.5, 700, 513) == T.E_UNSUPPORTED and bwd_act(act, 0.5, 700, 513) == T.E_UNSUPPORTED
        assert fwd_act(act, 0.5, -1, 16) == T.E_SHAPE and fwd_act(act, 0.5, 2 ** 31, 16) == T.E_RANGE
        assert fwd_act(act, 0.5, 0, 16) == 0 and bwd_act(act, 0.5, 0, 16) == 0
        assert bwd_act(act, 0.5, 700, 16, terms=9) == (T.E_RANGE if act == 0 else E_UNSUPPORTED)


def test_dispatch_does_not_depend_on_the_activation():
    seen = set()
    for act in CODES.values():
        for o in (4, 16, 24, 73, 128, 200):
            for n_rows in (T.BELOW, T.ABOVE):
                want_f, want_b = T.fwd(n_rows, o), T.bwd(n_rows, o)
                assert fwd_act(act, 0.2, n_rows, o) == want_f > 0, (act, o, n_rows)
                assert bwd_act(act, 0.2, n_rows, o) == want_b > 0, (act, o, n_rows)
                seen.update((want_f & 255, want_b & 255))
        for n_rows in (T.BELOW, T.ABOVE):                                # `out` one float off a 16-byte boundary
            assert fwd_act(act, 0.2, n_rows, 16, out=4) == T.fwd(n_rows, 16, out=4) == T.code(T.WAVE if n_rows == T.BELOW else T.GROUP, 1)
            assert bwd_act(act, 0.2, n_rows, 16, out=4) == T.bwd(n_rows, 16, out=4) == T.code(T.WAVE if n_rows == T.BELOW else T.GROUP, 1)
            g = T.graph(n_rows, col=True)                                # `col` present: edges not target-sorted
            assert fwd_act(act, 0.2, n_rows, 16, g=g) == T.fwd(n_rows, 16, g=g) == T.code(T.PF if n_rows == T.BELOW else T.GROUP, 4 if n_rows == T.BELOW else 1)
            assert bwd_act(act, 0.2, n_rows, 16, g=g) == T.bwd(n_rows, 16, g=g)
    assert seen == {T.PF, T.WAVE, T.GROUP, T.REC}                        # the cases reach every family


# ---- message_activation -----------------------------------------------------------------------------------------------------
def test_message_activation_recognises_the_listed_callables():
    from graph_odenet_amd.gat_layers import message_activation as ma
    relu, ident, leaky, elu, tanh, sig = (CODES[k] for k in ("RELU", "IDENTITY", "LEAKY_RELU", "ELU", "TANH", "SIGMOID"))
    for f in (F.relu, torch.relu, nn.ReLU()):
        assert ma(f) == (relu, 0.0)
    assert ma(F.elu) == (elu, 1.0) and ma(nn.ELU()) == (elu, 1.0) and ma(nn.ELU(alpha=0.5)) == (elu, 0.5)
    assert ma(F.leaky_relu) == (leaky, 0.01) and ma(nn.LeakyReLU()) == (leaky, 0.01) and ma(nn.LeakyReLU(0.2)) == (leaky, 0.2)
    for f in (torch.tanh, F.tanh, nn.Tanh()):
        assert ma(f) == (tanh, 0.0)
    for f in (torch.sigmoid, F.sigmoid, nn.Sigmoid()):
        assert ma(f) == (sig, 0.0)
    assert ma(nn.Identity()) == (ident, 0.0)
    assert ma(functools.partial(F.elu, alpha=0.25)) == (elu, 0.25) and ma(functools.partial(F.elu)) == (elu, 1.0)
    assert ma(functools.partial(F.leaky_relu, negative_slope=0.3)) == (leaky, 0.3)
    for code, param in (ma(nn.ELU(alpha=2)), ma(nn.LeakyReLU(1)), ma(functools.partial(F.elu, alpha=2))):
        assert type(code) is int and type(param) is float


def test_message_activation_gives_none_for_anything_else():
    from graph_odenet_amd.gat_layers import message_activation as ma

    class MyAct(nn.Module):
        def forward(self, v):
            return F.elu(v)

    class MyELU(nn.ELU):                                                 # a subclass may compute anything
        pass

    for f in (lambda v: F.elu(v), MyAct(), MyELU(), F.gelu, nn.GELU(), torch.exp, None, "elu",
              functools.partial(F.elu, inplace=True), functools.partial(F.elu, 1.0), functools.partial(F.leaky_relu, 0.2),
              functools.partial(F.relu), functools.partial(torch.clamp, min=0.0)):
        assert ma(f) is None, f


# ---- the comparisons bite -----------------------------------------------------------------------------------------------------
# A kernel is never made wrong on a GPU to see a test fail: the restatement is made wrong in the ways the new kernel code
# could be (test_gpu_gat_act.FAULTS) and held against itself under the GPU tests' metric and bound, on case S, o = 16.
def rejected(res):
    return sorted(q for q, (err, exact) in res.items() if not (err <= D.TOL and exact))


@pytest.mark.parametrize("fault,name,caught_by", [
    ("relu_derivative", "leaky_relu(0.2)", ["dPs", "dPt", "dz"]),                    # (a)
    ("alpha_ignored", "elu(0.5)", ["dA2", "dPs", "dPt", "da", "dz", "out"]),         # (b)
    ("forward_only", "elu", ["dA2", "dPs", "dPt", "da", "dz"]),                      # (c)
    ("zero_from_positive_branch", "leaky_relu(0.2)", ["dPs", "dPt", "dz"]),          # (d)
])
def test_each_fault_is_rejected_by_the_gpu_tests_comparisons(fault, name, caught_by):
    d, v = D.design("S"), D.values("S", True, 16)
    ref = A.reference(d, v, A.ACTS[name])
    assert D.passes(A.results_of(ref, ref))
    res = A.results_of(ref, A.reference(d, v, A.ACTS[name], fault=fault))
    print(fault, {q: "%.2e" % e for q, (e, _) in res.items()})
    assert rejected(res) == caught_by
    assert all(res[q][0] > 50 * D.TOL for q in caught_by)                            # far beyond the bound, not by a hair


def test_restatement_with_relu_is_the_designs_and_agrees_with_autograd():
    d, v = D.design("S", False), D.values("S", False, 7)
    ours, theirs = A.reference(d, v, (A.RELU, 0.0)), D.reference(d, v)
    for q in ("w", "den", "out", "dz", "da", "mag", "dPs", "dPt", "dA2", "magA2", "magPs", "magPt"):
        assert torch.equal(getattr(ours, q), getattr(theirs, q)), q
    s, t = torch.from_numpy(d.lut[d.src]), torch.from_numpy(d.lut[d.tgt])
    r, c = torch.from_numpy(d.lut[d.rows]), torch.from_numpy(d.cols)
    val, na = torch.from_numpy(d.vals).double(), v.Ps.shape[0]
    acts = {"identity": lambda z: z, "leaky_relu": F.leaky_relu, "leaky_relu(0.2)": lambda z: F.leaky_relu(z, 0.2), "elu": F.elu,
            "elu(0.5)": lambda z: F.elu(z, 0.5), "tanh": torch.tanh, "sigmoid": torch.sigmoid}
    for name, fn in acts.items():                                        # torch's own activation and autograd, z == 0 included
        ref = A.reference(d, v, A.ACTS[name])
        Ps, Pt, A2 = (x.double().requires_grad_() for x in (v.Ps, v.Pt, v.A2))
        a = (A2[s, 0] + A2[t, 1]) + v.bw.double()
        a = a + (ref.a32.double() - a).detach()
        w = torch.exp(a - ref.amax.double())                             # the maximum held fixed: no max path
        y = fn(Ps[s] + Pt[t] + v.bf.double())
        we = val * w[c]
        den = torch.zeros(na, dtype=torch.float64).index_add(0, r, we) + D.EPS
        out = torch.zeros(na, 7, dtype=torch.float64).index_add(0, r, we[:, None] * y[c]) / den[:, None]
        assert torch.allclose(out, ref.out, rtol=1e-12, atol=1e-300), name
        gPs, gPt, gA2 = torch.autograd.grad(out, (Ps, Pt, A2), v.dout.double())
        for got, want in ((gPs, ref.dPs), (gPt, ref.dPt)):
            assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item(), name
        assert (gA2 - ref.dA2).abs().max().item() <= 1e-12 * ref.magA2.max().item(), name
        assert (ref.z == 0).any()


@pytest.mark.parametrize("kind,o", [("S", 16), ("B1", 32)])
def test_fp32_arithmetic_alone_stays_within_a_quarter_of_the_bound(kind, o):
    """Why every activation keeps D.TOL: a float32 torch restatement is within D.TOL / 4 of float64 under the metric (the
    figures are in test_gpu_gat_act.py's docstring)."""
    d, v = D.design(kind), D.values(kind, True, o)
    for name, act in A.ACTS.items():
        res = A.results_of(A.reference(d, v, act), A.reference(d, v, act, dtype=torch.float32))
        worst = max(err for err, _ in res.values())
        print("%s o=%d %-16s fp32 vs fp64: worst %.2e  %s" % (kind, o, name, worst, {q: "%.1e" % e for q, (e, _) in res.items()}))
        assert worst <= D.TOL / 4 and all(exact for _, exact in res.values()), (name, res)
