"""The message activation of the fused GAT ODE function on the CPU (graphode.h: gode_gat_act_t with outer_relu set on the
five gode_gat_agg_* entry points, and `act, act_param` at the end of gode_gat_odefunc_t): the symbols and their
signatures, the checks that come first, the dispatch (it does not depend on the activation, with or without cotangent
terms), the refusal the backward keeps without the outer relu, and the plan token of the two ODE functions.  Nothing is
launched: every call either is a route query or returns a validation code, so the pointers are made up
(test_gat_routes.py's, test_gat_backprop_abi.py's).
"""
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gat_routes as T                                             # noqa: E402  (made-up pointers, graph(), proj())
import test_gat_act_abi as A                                            # noqa: E402  (the same arguments without the outer relu)
import test_gat_backprop_abi as B                                       # noqa: E402  (a made-up odefunc / workspace pair)

from graph_odenet_amd import _lib                                       # noqa: E402

E_NULLPTR, E_SHAPE, E_RANGE, E_UNSUPPORTED = -1, -2, -4, -5
CODES = A.CODES
P, vp = T.P, T.vp
NAN, INF = float("nan"), float("inf")


def test_symbols_signatures_and_struct():
    lib = _lib.load()
    sig = _lib.SIGNATURES
    for name in ("gode_gat_agg_ode_f32_fwd", "gode_gat_agg_ode_f32_fwd_route", "gode_gat_agg_ode_f32_bwd",
                 "gode_gat_agg_ode_f32_bwd_route", "gode_gat_agg_heads_ode_f32_fwd"):
        assert name in A.GONE and name not in sig and not hasattr(lib, name), name
    for name, argtypes in A.want_signatures().items():                   # outer_relu rides the one activation argument
        assert hasattr(lib, name) and sig[name] == (ctypes.c_int, argtypes), name
    assert _lib.GatAct._fields_[2] == ("outer_relu", ctypes.c_int32) and ctypes.sizeof(_lib.GatAct) == 12
    assert len(_lib.STRUCTS) == 11
    fields = _lib.GatOdeFunc._fields_
    assert [f[0] for f in fields[-3:]] == ["Wpacked", "act", "act_param"]
    assert fields[-2][1] is ctypes.c_int32 and fields[-1][1] is ctypes.c_float
    fs = _lib.GatOdeFunc()
    assert fs.act == CODES["RELU"] and fs.act_param == 0.0               # a zeroed struct is relu


# ---- the aggregation entry points on test_gat_routes.py's made-up arguments -----------------------------------------------
def fwd_ode(act, param, n_rows, o, out=0, g=None, launch=False):
    return T.fwd(n_rows, o, out=out, g=g, act=_lib.GatAct(act, param, 1), launch=launch)


def bwd_ode(act, param, n_rows, o, terms=0, out=0, term=0, g=None, launch=False, old=False):
    """old: without the outer relu (what gode_gat_agg_act_f32_bwd was).  T.bwd asserts that the flag is untouched: neither
    a query nor a refused call writes it."""
    return T.bwd(n_rows, o, terms, out=out, term=term, g=g, act=_lib.GatAct(act, param, 0 if old else 1), launch=launch)


def test_the_activation_checks_come_first_then_the_old_checks_in_their_order():
    lib = _lib.load()
    for launch in (False, True):                                         # the launching calls answer the same before any launch
        for act in (-1, 6, 1 << 20):
            assert fwd_ode(act, 0.0, 700, 16, launch=launch) == E_SHAPE
            assert bwd_ode(act, 0.0, 700, 16, launch=launch) == E_SHAPE and bwd_ode(act, 0.0, 700, 16, terms=3, launch=launch) == E_SHAPE
        for act in (CODES["LEAKY_RELU"], CODES["ELU"]):
            for bad in (NAN, INF, -INF):
                assert fwd_ode(act, bad, 700, 16, launch=launch) == E_SHAPE and bwd_ode(act, bad, 700, 16, terms=1, launch=launch) == E_SHAPE
    nulls_f = (None, None, None, None, 16, None, None, None, 0.0, None, None, None)
    nulls_b = (None, None, None, None, 16, None, None, None, None, None, None, 1.0, None, None, None, 16, None, 2, None)
    nulls_h = (None, None, None, None, 16, None, None, None, 9000, 8, 0.0, None, None, None)
    mode = lambda act, param: ctypes.byref(_lib.GatAct(act, param, 1))   # noqa: E731
    for fn, nulls in ((lib.gode_gat_agg_f32_fwd, nulls_f), (lib.gode_gat_agg_f32_fwd_route, nulls_f),
                      (lib.gode_gat_agg_f32_bwd, nulls_b), (lib.gode_gat_agg_f32_bwd_route, nulls_b),
                      (lib.gode_gat_agg_heads_f32_fwd, nulls_h)):
        for act in (-1, 6):
            assert fn(*nulls, mode(act, 0.0), None) == E_SHAPE           # before any pointer is looked at
        assert fn(*nulls, mode(CODES["ELU"], NAN), None) == E_SHAPE and fn(*nulls, mode(CODES["LEAKY_RELU"], INF), None) == E_SHAPE
        assert fn(*nulls, mode(CODES["ELU"], 1.0), None) == E_NULLPTR    # then the old entry's checks, with its codes
        assert fn(*nulls, mode(CODES["TANH"], NAN), None) == E_NULLPTR   # a parameter nobody reads may be anything
        assert fn(*nulls, None, None) == E_NULLPTR                       # and no struct at all is relu
    # the heads form: the old checks in the old order behind the new one
    g, p = T.graph(700), T.proj(8)
    def heads(act, o=8, heads=8, n_edges=9000, scratch=True):            # noqa: E306
        return lib.gode_gat_agg_heads_f32_fwd(ctypes.byref(g), vp(P["src"]), vp(P["tgt"]), ctypes.byref(p), o, vp(P["bf"]),
                                              vp(P["a"]), vp(P["scratch"]) if scratch else None, n_edges, heads, 1e-9,
                                              vp(P["out"]), vp(P["w"]), vp(P["den"]), mode(act, 1.0), None)
    for act in CODES.values():
        assert heads(act, scratch=False) == E_NULLPTR and heads(act, heads=0) == E_SHAPE and heads(act, n_edges=-1) == E_SHAPE
        assert heads(act, heads=65) == E_UNSUPPORTED and heads(act, o=513) == E_UNSUPPORTED
        assert heads(6, heads=65) == E_SHAPE
    # the one-head forms: the old entry's validation codes come back unchanged, under every activation
    for act in CODES.values():
        assert fwd_ode(act, 0.5, 700, 513) == E_UNSUPPORTED and bwd_ode(act, 0.5, 700, 513, terms=2) == E_UNSUPPORTED
        assert fwd_ode(act, 0.5, -1, 16) == E_SHAPE and fwd_ode(act, 0.5, 2 ** 31, 16) == E_RANGE
        assert fwd_ode(act, 0.5, 0, 16) == 0 and bwd_ode(act, 0.5, 0, 16, terms=3) == 0
        assert bwd_ode(act, 0.5, 700, 16, terms=9) == E_RANGE             # too many terms: the cotangent's own check, not a refusal


def test_routes_are_the_act_routes_with_and_without_cotangent_terms():
    seen = set()
    for act in CODES.values():
        for o in (4, 16, 24, 73, 128, 200):
            for n_rows in (T.BELOW, T.ABOVE):
                assert fwd_ode(act, 0.2, n_rows, o) == A.fwd_act(act, 0.2, n_rows, o) == T.fwd(n_rows, o) > 0, (act, o, n_rows)
                assert bwd_ode(act, 0.2, n_rows, o) == A.bwd_act(act, 0.2, n_rows, o) == T.bwd(n_rows, o) > 0, (act, o, n_rows)
                for terms in (1, 3):                                     # relu's route; refused without the outer relu
                    want = T.bwd(n_rows, o, terms)
                    assert bwd_ode(act, 0.2, n_rows, o, terms=terms) == want > 0, (act, o, n_rows, terms)
                    assert bwd_ode(act, 0.2, n_rows, o, terms=terms, term=4) == T.bwd(n_rows, o, terms, term=4) > 0
                    seen.add(want & 255)
                    if act != CODES["RELU"]:
                        assert A.bwd_act(act, 0.2, n_rows, o, terms=terms) == E_UNSUPPORTED
        for n_rows in (T.BELOW, T.ABOVE):                                # `out` one float off a 16-byte boundary; `col` present
            assert fwd_ode(act, 0.2, n_rows, 16, out=4) == T.fwd(n_rows, 16, out=4)
            assert bwd_ode(act, 0.2, n_rows, 16, terms=3, out=4) == T.bwd(n_rows, 16, 3, out=4) == T.code(T.WAVE, 1)
            g = T.graph(n_rows, col=True)
            assert fwd_ode(act, 0.2, n_rows, 16, g=g) == T.fwd(n_rows, 16, g=g)
            assert bwd_ode(act, 0.2, n_rows, 16, terms=1, g=g) == T.bwd(n_rows, 16, 1, g=g)
    assert seen == {T.PF, T.WAVE, T.REC}                                 # the masked cotangent has no lane-group form
    # an unaligned last term leaves the prefetched and the record route for the wave kernel
    assert T.bwd(T.BELOW, 16, 3, term=4) == T.code(T.WAVE, 1) and T.bwd(T.ABOVE, 16, 3, term=4) == T.code(T.WAVE, 1)


def test_the_old_act_backward_still_refuses_cotangent_terms():
    for launch in (False, True):
        for act in (1, 2, 3, 4, 5):
            for terms in (1, 3):
                assert bwd_ode(act, 0.5, 700, 16, terms=terms, launch=launch, old=True) == E_UNSUPPORTED
    assert bwd_ode(CODES["RELU"], 0.0, 700, 16, terms=3, old=True) == T.bwd(700, 16, 3) > 0


# ---- act, act_param in gode_gat_odefunc_t: every gode_gat_ode_* entry point ---------------------------------------------------
def _ode_calls(fs, ws):
    """Every gode_gat_ode_* entry point that takes the struct, on arguments that pass every check but the struct's."""
    lib = _lib.load()
    b = [B._buf() for _ in range(12)]
    k7 = [B._buf() for _ in range(7)]
    yb = [B._buf() for _ in range(7)]
    A7 = lambda: B._ptr_array(k7)                                        # noqa: E731
    f, w = ctypes.byref(fs), ctypes.byref(ws)
    sums = (ctypes.c_double * 4)()
    yb4 = (ctypes.c_void_p * 4)(*[B.P(x) for x in yb[:4]])
    keep = (b, k7, yb, sums, yb4)
    calls = {
        "dopri5_step_forward": lambda: lib.gode_gat_ode_dopri5_step_forward(
            f, B.P(b[0]), A7(), B.P(b[1]), w, 0.0, 0.1, 1e-3, 1e-3, sums, B.P(b[2]), None),
        "dopri5_step_adjoint": lambda: lib.gode_gat_ode_dopri5_step_adjoint(
            f, B.P(b[0]), B.P(b[1]), B.P(b[2]), B.P(b[3]), A7(), A7(), A7(), A7(), B.P(b[4]), B.P(b[5]), B.P(b[6]), B.P(b[7]), w,
            0.0, 0.1, 1e-3, 1e-3, sums, B.P(b[8]), None),
        "rk4_forward_save": lambda: lib.gode_gat_ode_rk4_forward_save(*B._forward_save_args(fs, ws, b)),
        "rk4_backprop": lambda: lib.gode_gat_ode_rk4_backprop(*B._rk4_backprop_args(fs, ws, b, yb[:4])),
        "dopri5_step_backprop": lambda: lib.gode_gat_ode_dopri5_step_backprop(*B._dopri5_args(fs, ws, b, k7, yb)),
    }
    for m, name in ((_lib.CONSTANTS["GODE_RK_EULER"], "euler"), (_lib.CONSTANTS["GODE_RK_MIDPOINT"], "midpoint"),
                    (_lib.CONSTANTS["GODE_RK_RK4_38"], "rk4")):
        calls["fixed_forward_save " + name] = lambda m=m: lib.gode_gat_ode_fixed_forward_save(
            m, f, B.P(b[0]), B.P(b[1]), B.P(b[2]), w, 0.0, 1.0, 4, 0, 4, None)
        calls["fixed_backprop " + name] = lambda m=m: lib.gode_gat_ode_fixed_backprop(
            m, f, B.P(b[0]), B.P(b[1]), B.P(b[2]), yb4, B.P(b[3]), B.P(b[4]), w, 0.0, 1.0, 4, 0, 4, None)
    return calls, keep


def test_a_bad_activation_in_the_struct_is_refused_by_every_ode_entry_point():
    for heads, d in ((1, 16), (8, 64)):
        for act, param in ((6, 0.0), (-1, 0.0), (CODES["ELU"], NAN), (CODES["LEAKY_RELU"], INF), (CODES["ELU"], -INF)):
            fs, ws, _keep = B._structs(d=d, heads=heads)
            fs.act, fs.act_param = act, param
            calls, _k = _ode_calls(fs, ws)
            assert len(calls) == 11
            for name, call in calls.items():
                assert call() == E_SHAPE, (name, act, param, heads)
    # before anything else of the struct: one that every other check refuses with another code
    for act in (6, -1):
        fs, ws, _keep = B._structs(d=128)                                # GODE_E_UNSUPPORTED from the sweeps otherwise
        fs.act, fs.Wlog = act, None                                      # GODE_E_NULLPTR from check_common otherwise
        calls, _k = _ode_calls(fs, ws)
        for name, call in calls.items():
            assert call() == E_SHAPE, (name, act)
    # and a good activation leaves the other refusals as they were (a parameter nobody reads may be anything)
    for act, param in ((CODES["ELU"], 1.0), (CODES["TANH"], NAN), (CODES["RELU"], NAN)):
        fs, ws, _keep = B._structs(d=128)
        fs.act, fs.act_param = act, param
        calls, _k = _ode_calls(fs, ws)
        for name, call in calls.items():
            if "dopri5_step_forward" in name or "dopri5_step_adjoint" in name:
                continue                                                 # no sweep check there: they would launch
            assert call() == E_UNSUPPORTED, (name, act)
        fs.Wlog = None
        for name, call in calls.items():
            assert call() == E_NULLPTR, (name, act)


# ---- Python: the spec's activation and the plan token -------------------------------------------------------------------------
def _tiny_graph():
    g = torch.Generator().manual_seed(0)
    n, E = 10, 30
    src = torch.randint(0, n, (E,), generator=g)
    tgt = torch.randint(0, n, (E,), generator=g).sort().values
    M = torch.sparse_coo_tensor(torch.stack([tgt, torch.arange(E)]), torch.ones(E), (n, E)).coalesce()
    return n, src, tgt, M


def test_plan_token_carries_the_activation():
    from graph_odenet_amd import gat_heads, gat_models
    n, src, tgt, M = _tiny_graph()
    y0 = torch.zeros(n, 16)
    for make in (lambda act: gat_models.ODEfunc(16, act=act), lambda act: gat_heads.ODEfunc(16, heads=2, act=act)):
        f = make(F.elu)
        f.set_adj(src, tgt, M)
        elu = f.gode_plan_token(y0)
        f.gc1.act = torch.tanh
        tanh = f.gode_plan_token(y0)
        f.gc1.act = F.elu
        assert elu != tanh and f.gode_plan_token(y0) == elu and hash(elu) != hash(tanh)
        assert elu[-1] == (CODES["ELU"], 1.0) and tanh[-1] == (CODES["TANH"], 0.0)
        f.gc1.act = torch.nn.ELU(alpha=0.5)
        assert f.gode_plan_token(y0) not in (elu, tanh)                  # the parameter counts as well
        relu = make(F.relu)
        relu.set_adj(src, tgt, M)
        assert relu.gode_plan_token(y0)[-1] == (CODES["RELU"], 0.0)


def test_default_signature_and_state_dict_are_the_references():
    from graph_odenet_amd import gat_heads, gat_models
    a, b = gat_models.ODEfunc(16), gat_models.ODEfunc(16, act=F.elu)
    assert a.gc1.act is F.relu and b.gc1.act is F.elu and list(a.state_dict()) == list(b.state_dict())
    a, b = gat_heads.ODEfunc(16, 2), gat_heads.ODEfunc(16, heads=2, act=torch.tanh)
    assert a.gc1.act is F.relu and b.gc1.act is torch.tanh and all(hd.act is torch.tanh for hd in b.gc1.heads)
    assert list(a.state_dict()) == list(b.state_dict())


def test_train_res_act_option():
    from graph_odenet_amd import gat_models, train_res
    p = train_res.build_parser()
    assert p.parse_args([]).act == "relu"
    assert sorted(train_res.ODE_ACTS) == ["elu", "identity", "leaky_relu", "relu", "sigmoid", "tanh"]
    from graph_odenet_amd.gat_layers import message_activation
    assert sorted(message_activation(f)[0] for f in train_res.ODE_ACTS.values()) == [0, 1, 2, 3, 4, 5]
    f = gat_models.ODEfunc(16)
    holder = torch.nn.Sequential(f)
    train_res.set_ode_act(holder, train_res.ODE_ACTS["elu"])
    assert f.gc1.act is F.elu
