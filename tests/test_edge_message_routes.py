"""The design of the QC edge-message route tests, checked on the CPU: every case of edge_message_routes_design.py reaches the
routes its entry names (recomputed here from the design's written-out limits, which are asserted textually against the
sources), the tables together reach every route, the exact data stays below 2^24 granules and is reproduced bit for bit by
plain float32 arithmetic, plain float32 stays a factor 4 inside the tolerances on the real data, the eight entry points
answer their host-side range, shape, alias and null checks through the C ABI (nothing is launched, so the pointers are made
up), and nine deliberately altered copies of the float64 restatement are each rejected by both comparisons the GPU tests use.
No GPU.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_message_routes_design as D                                  # noqa: E402

from graph_odenet_amd import _lib                                       # noqa: E402

NAMES = ("rowptr", "eid", "val", "src", "A", "X", "out", "msg", "edge_row", "edge_val", "dM", "dA", "dxe", "S", "bias", "k", "fout",
         "dS", "ms_rowptr", "ms_eid", "t0", "t1", "w")
P = {name: 0x10000 * (k + 1) for k, name in enumerate(NAMES)}


def vp(name):
    return None if name is None or name is True else ctypes.c_void_p(P[name])


# ---- limits ----------------------------------------------------------------------------------------------------------------
def test_limits_are_the_sources():
    """The numbers the design states are the ones in the kernels' sources and in ops.py."""
    from graph_odenet_amd import ops
    root = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    edge, ode = (open(os.path.join(root, f)).read() for f in ("edge.hip", "edge_ode.hip"))
    assert "constexpr int kMsgTile = %d;" % D.MSG_TILE in edge
    assert edge.count("const int rpt = kMsgTile / h > 0 ? kMsgTile / h : 1") == 2            # the fused and the per-edge kernel
    assert "if (h <= %d) {\n        hipLaunchKernelGGL(edge_matvec_fwd_kernel<1>" % D.MSG_XP_MAX_H in edge
    assert "hipLaunchKernelGGL(edge_matvec_fwd_kernel<16>" in edge
    assert edge.count("h > %d) return GODE_E_RANGE;" % D.MSG_HMAX) == 3
    assert "const size_t lds = (size_t)(2 * ((h + 3) & ~(int64_t)3) + (rpt < h ? rpt : h) * h) * sizeof(float);" in edge
    assert "for (; j + %d <= h; j += %d)" % (D.MSG_UNROLL, D.MSG_UNROLL) in edge
    assert "for (; i + %d <= h; i += %d)" % (D.MSG_UNROLL, D.MSG_UNROLL) in edge
    assert "__shared__ int es[%d], ss[%d];" % (D.ROUND, D.ROUND) in edge and "base += %d" % D.ROUND in edge
    assert "const int cnt = min(%d, ne - base), T = cnt * ntiles;" % D.ROUND in edge
    for text in (edge, ode):
        assert "h > %d) return GODE_E_RANGE;" % D.OUTER_HMAX in text
        assert "n_terms < 1 || n_terms > GODE_MAX_TERMS) return GODE_E_RANGE;" in text
        assert "const size_t lds = (size_t)2 * n_terms * h * sizeof(float);" in text
        assert "lds > 48 * 1024" in text and D.LDS_DEFAULT == 48 * 1024
    assert "constexpr int kEdgeOdeMaxH = %d;" % D.ODE_HMAX in ode and "constexpr int kVjpRound = %d;" % D.VJP_ROUND in ode
    (h1, p1), (h2, p2), (h3, p3) = D.ODE_PF
    assert "if (h <= %d) GODE_EF(%d) else if (h <= %d) GODE_EF(%d) else GODE_EF(%d)" % (h1, p1, h2, p2, p3) in ode and h3 == D.ODE_HMAX
    assert "const size_t lds = (size_t)(h + h * (h + 1)) * sizeof(float);" in ode
    assert "__shared__ int es[%d], ss[%d];" % (D.ROUND, D.ROUND) in ode and "const int cnt = min(%d, ne - base);" % D.ROUND in ode
    assert "for (; j + %d <= h; j += %d)" % (D.FEVAL_UNROLL, D.FEVAL_UNROLL) in ode
    assert "const int G = %d / hp" % D.THREADS in ode and "for (; i + %d <= i1; i += %d)" % (D.MSG_UNROLL, D.MSG_UNROLL) in ode
    assert "const int rpg = (h + G - 1) / G, i0 = min(h, grp * rpg), i1 = min(h, i0 + rpg);" in ode
    assert "return fout[idx] > 0.f ? g : 0.f;" in open(os.path.join(root, "common.h")).read()
    assert _lib.GODE_MAX_TERMS == D.MAX_TERMS
    header = " ".join(open(_lib.HEADER_PATH).read().split())
    for name, value in (("NULLPTR", D.E_NULLPTR), ("SHAPE", D.E_SHAPE), ("RANGE", D.E_RANGE)):
        assert "#define GODE_E_%s (%d)" % (name, value) in header
    # the public functions' thresholds: the GPU cases at 255 | 256 and 4095 | 4096 edges are only about them while they read so
    assert ops.EDGE_MSG_MIN_EDGES == D.EDGE_MSG_MIN_EDGES == 256 and ops.EDGE_ODE_FUSED_MAX_EDGES == D.EDGE_ODE_FUSED_MAX_EDGES == 4096
    assert D.PUBLIC_MESSAGE_EDGES == (255, 256) and D.PUBLIC_FIELD_EDGES == (4095, 4096)


def test_limits_rederived():
    assert [D.msg_tiles(h) for h in (90, 91, 129)] == [(91, 1, 90), (90, 2, 1), (63, 3, 3)]
    assert [D.msg_tiles(h)[1] for h in (1, 73, 128, 255, 256, 257, 4096)] == [1, 1, 2, 8, 8, 9, 2048]
    assert min(h for h in range(1, D.MSG_HMAX + 1) if D.matvec_lds(h) > D.LDS_DEFAULT) == 2457
    assert D.matvec_lds(2456) == 49120 and D.matvec_lds(4096) == 64 * 1024 == max(D.matvec_lds(h) for h in range(1, D.MSG_HMAX + 1))
    assert all(D.matvec_lds(h) <= D.LDS_DEFAULT for h in range(1, D.MSG_XP_MAX_H + 1))        # <1> never needs the opt-in
    # the per-edge kernels never need it: h + min(rpt, h) h floats, and 2 h floats
    assert max((h + min(D.msg_tiles(h)[0], h) * h) * 4 for h in range(1, D.MSG_HMAX + 1)) == D.LDS_DEFAULT
    assert min(h for h in range(1, D.ODE_HMAX + 1) if D.feval_lds(h) > D.LDS_DEFAULT) == 110
    assert all(h * h <= D.feval_pf(h) * D.THREADS for h in range(1, D.ODE_HMAX + 1))            # the prefetch registers hold A_e
    assert [D.feval_pf(h) for h in (32, 33, 64, 65, 112)] == [4, 16, 16, 49, 49]
    assert D.OUTER_OPTIN * 8 == D.LDS_DEFAULT and 8 * 768 == D.OUTER_OPTIN < 8 * 769
    assert D.vjp_groups(1)[:3] == (1, 256, 1) and D.vjp_groups(33)[:3] == (64, 4, 9) and D.vjp_groups(33)[3] == [9, 9, 9, 6]
    assert D.vjp_groups(65)[:3] == (128, 2, 33) and D.vjp_groups(112)[3] == [56, 56] and D.vjp_groups(96)[:3] == (128, 2, 48)
    assert all(sum(D.vjp_groups(h)[3]) == h for h in range(1, D.ODE_HMAX + 1))                  # every row has one group
    assert (D.VJP_ROUND * D.ODE_HMAX + 256) * 4 <= D.LDS_DEFAULT


# ---- routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.ALL_CASES, ids=lambda c: "%s/%s" % (c.family, c.name))
def test_every_case_reaches_its_routes(case):
    got = case.route()
    assert case.reaches and case.reaches <= got, (case.name, case.reaches - got)
    b = case.batch
    assert b.E * case.h * case.h <= 3 * 4096 * 4096 and b.n <= 15                              # nothing needs the workload's sizes
    if case.sorted_by == "tgt":
        assert b.eid.tolist() == list(range(b.E))
    elif case.sorted_by == "src":
        assert b.ms_eid.tolist() == list(range(b.E))
    else:
        assert b.E <= 3 or (b.eid.tolist() != sorted(b.eid.tolist()) and b.ms_eid.tolist() != sorted(b.ms_eid.tolist()))
    assert (b.tgt < 0).sum().item() == (2 if case.negrows else 0)


def test_tables_are_the_issues():
    by = D.BY_NAME
    assert D.MATVEC_WIDTHS == (1, 3, 7, 8, 9, 15, 16, 17, 73, 90, 91, 128, 129, 255, 256, 257, 300)
    assert D.ODE_WIDTHS == (1, 3, 4, 5, 16, 31, 32, 33, 63, 64, 65, 96, 109, 110, 111, 112)
    for fam, widths in (("matvec", D.MATVEC_WIDTHS), ("feval", D.ODE_WIDTHS), ("vjp", D.ODE_WIDTHS)):
        for h in widths:
            c = by[fam, "width%d" % h]
            assert c.h == h and c.kind == "plain" and (c.batch.n, c.batch.E) == (12, 40) and not (c.strided or c.noval or c.negrows)
    plain = D.batch("plain")
    assert plain.in_degrees[-1] == 0 and max(plain.in_degrees) >= 9 and {d % 2 for d in plain.in_degrees if d} == {0, 1}
    ind, outd = D.batch("indeg"), D.batch("outdeg")
    assert ind.in_degrees[0::2] == list(D.IN_DEGREES) == [513, 0, 1, 2, 3, 255, 256, 257] and set(ind.in_degrees[1::2]) == {0}
    assert outd.out_degrees[0::2] == list(D.OUT_DEGREES) == [33, 0, 1, 15, 16, 17] and set(outd.out_degrees[1::2]) == {0}
    assert ind.in_degrees[0] and ind.in_degrees[-1] and outd.out_degrees[0] and outd.out_degrees[-1]      # atom 0 and the last atom
    assert {(c.h, c.kind) for c in D.MATVEC_CASES if c.kind == "indeg"} == {(16, "indeg"), (91, "indeg")}
    assert {c.h for c in D.MATVEC_CASES if c.fwd_only} == {2456, 2457, 4096} and all(c.batch.E == 3 for c in D.MATVEC_CASES if c.fwd_only)
    assert sorted(d for d in D.batch("three").in_degrees if d) == [1, 2]
    assert {c.h for c in D.MATVEC_CASES if c.strided} == {73, 257}
    assert {c.h for c in D.MATVEC_CASES if c.sorted_by} == {16, 91} == {c.h for c in D.MATVEC_CASES if c.noval and not c.negrows}
    assert any(c.negrows and c.noval for c in D.MATVEC_CASES)
    outer = {(c.n_terms, c.h) for c in D.OUTER_CASES}
    assert {(n, 73) for n in (1, 2, 3, 4, 7, 8)} | {(2, h) for h in (1, 16, 255, 256, 257)} | {(8, 768), (8, 769), (8, 1024)} <= outer
    assert any(c.negrows and c.noval for c in D.OUTER_CASES) and any(c.strided for c in D.OUTER_CASES)
    assert all(c.batch.E == 3 for c in D.OUTER_CASES if c.h >= 768)
    for n in (2, 3, 4, 7, 8):
        w = D.outer_weights(n)
        assert len(w) == n and 0.0 in w and min(w) < 0
    assert D.outer_weights(1) == [-0.5] and D.outer_weights(2) == [0.0, -0.5]
    widths = lambda cases: [c for c in cases if c.name.startswith("width")]                          # noqa: E731
    assert {(c.n_terms, c.alpha) for c in widths(D.FEVAL_CASES)} == {(n, a) for n in (0, 1, 3, 8) for a in (1.0, -0.5, 0.25)}
    assert {(c.n_terms, c.cot_scale) for c in widths(D.VJP_CASES)} == {(n, s) for n in (1, 3, 8) for s in (1.0, -1.0, 0.5)}
    assert {c.h for c in D.FEVAL_CASES if c.kind == "indeg"} == {16, 65}
    assert any(c.sorted_by == "tgt" for c in D.FEVAL_CASES) and any(c.noval for c in D.FEVAL_CASES)
    assert any(c.kind == "outdeg" and not c.sorted_by for c in D.VJP_CASES) and any(c.sorted_by == "src" for c in D.VJP_CASES)
    assert any(c.noval for c in D.VJP_CASES) and sum(c.negrows for c in D.VJP_CASES) == 2


def test_tables_reach_every_route():
    reached = {fam: set() for fam in ("matvec", "outer", "feval", "vjp")}
    for c in D.ALL_CASES:
        reached[c.family] |= c.route()
    need = {
        "matvec": {"tiles1", "tiles2", "tiles3+", "XP1", "XP16", "lds_default", "lds_optin", "lds==64K", "tail_only", "last_tile_one_row",
                   "last_tile_short", "rounds0", "rounds1", "rounds2", "rounds3", "rounds_full_last", "T==1", "T_odd", "T_even",
                   "tiles>1&T_odd", "tiles>1&T_even"} | {"h%%8==%d" % r for r in range(8)},
        "outer": {"terms%d" % n for n in (1, 2, 3, 4, 7, 8)} | {"lds_default", "lds_optin"},
        "feval": {"PF4", "PF16", "PF49", "PF_full", "lds_default", "lds_optin", "rounds0", "rounds1", "rounds2", "rounds3",
                  "rounds_full_last"} | {"h%%4==%d" % r for r in range(4)},
        "vjp": {"hp%d" % p for p in (1, 4, 8, 16, 32, 64, 128)} | {"G%d" % g for g in (256, 64, 32, 16, 8, 4, 2)}
        | {"unrolled", "unrolled_tail", "tail_only", "empty_groups", "short_last_group", "idle_columns", "vrounds0", "vrounds1",
           "vrounds2", "vrounds3", "vrounds_full_last"}}
    for fam, tags in need.items():
        assert tags <= reached[fam], (fam, tags - reached[fam])
    # the opt-in on each side of its boundary, per kernel that has one
    sides = lambda fam: {(c.h, "lds_optin" in c.route()) for c in D.ALL_CASES if c.family == fam}      # noqa: E731
    assert {(2456, False), (2457, True), (4096, True)} <= sides("matvec") and {(109, False), (110, True)} <= sides("feval")
    assert {(768, False), (769, True)} <= sides("outer")
    # in-degrees above one round at one tile per edge and at two; PF classes with the round loop
    assert {"rounds3", "tiles1"} <= D.BY_NAME["matvec", "indeg_h16"].route() and {"rounds3", "tiles2"} <= D.BY_NAME["matvec", "indeg_h91"].route()
    assert {"rounds3", "PF4"} <= D.BY_NAME["feval", "indeg_h16"].route() and {"rounds3", "PF49"} <= D.BY_NAME["feval", "indeg_h65"].route()
    # a source with more than 16 edges where the unrolled loop runs with a tail, and where it does not run
    assert {"vrounds3", "unrolled_tail"} <= D.BY_NAME["vjp", "outdeg_h65"].route() and {"vrounds3", "tail_only"} <= D.BY_NAME["vjp", "outdeg_h16"].route()
    # two tiles make T = 2 cnt even whatever the degree: an odd T with several tiles needs an odd number of tiles
    assert "tiles>1&T_odd" not in D.BY_NAME["matvec", "indeg_h91"].route() and D.msg_tiles(129)[1] % 2 == 1


# ---- the data --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.ALL_CASES, ids=lambda c: "%s/%s" % (c.family, c.name))
def test_exact_data_is_exact_and_real_data_is_well_conditioned(case):
    d = D.inputs(case, "exact")
    assert D.exact_bound(case, d) < 2 ** 24
    g = D.granularity(case)
    ref = D.reference(case, d)
    assert all(torch.equal(t / g, torch.round(t / g)) for t in ref.values())
    assert not D.unequal(D.reference(case, d, torch.float32), ref)          # summation order does not matter below 2^24
    assert all(t.abs().max().item() > 0 for k, t in ref.items() if not (k == "k" and case.h == 1))
    if case.noval:
        assert torch.equal(d["ev"], torch.ones(case.batch.E))
    else:
        assert set(d["ev"].tolist()) <= {1.0, 2.0, 3.0}
    if case.family == "vjp":
        f = d["fout"]
        assert (f > 0).any() and (f < 0).any() and ((f == 0) & ~torch.signbit(f)).any() and ((f == 0) & torch.signbit(f)).any()
    d = D.inputs(case, "real")
    ref = D.reference(case, d)
    e32 = D.errors(D.reference(case, d, torch.float32), ref)
    assert set(e32) == set(ref) and all(4.0 * e <= D.tolerance(k) for k, e in e32.items()), e32
    if case.family == "vjp":
        f = d["fout"]
        assert ((f == 0) & ~torch.signbit(f)).any() and ((f == 0) & torch.signbit(f)).any()


def test_strided_blocks_are_surrounded_by_nan():
    t = torch.arange(12.0).reshape(4, 3)
    full, view = D.strided_block(t)
    assert view.stride() == (3 + D.PAD, 1) and view.storage_offset() == 1 and torch.equal(view, t)
    assert torch.isnan(full[:, 0]).all() and torch.isnan(full[:, 4:]).all()


def test_comparisons_reject_nan_shape_and_one_entry():
    case = D.BY_NAME["matvec", "width9"]
    ref = D.reference(case, D.inputs(case, "real"))
    got = {k: v.clone() for k, v in ref.items()}
    assert not D.failures(D.errors(got, ref)) and not D.unequal(got, ref)
    got["out"][3, 8] += 3e-5 * max(1.0, ref["out"].abs().max().item())
    got["dxe"][39, 8] += 3e-5 * max(1.0, ref["dxe"].abs().max().item())
    assert D.failures(D.errors(got, ref)) == ["out", "dxe"] and D.unequal(got, ref) == ["out", "dxe"]
    got["out"][3, 8] = float("nan")
    got["dxe"] = ref["dxe"][:, :8]
    assert D.failures(D.errors(got, ref)) == ["out", "dxe"] and D.unequal(got, ref) == ["out", "dxe"]


# ---- host-side answers through the ABI -----------------------------------------------------------------------------------
def lincomb(n, null_at=None):
    lc = _lib.LinComb()
    lc.n = n
    for j in range(min(n, D.MAX_TERMS)):
        lc.coef[j] = 1.0
        lc.ptr[j] = 0 if j == null_at else P["t0"] + 64 * j
    return lc


def fwd(h=16, n_rows=4, ldx=None, ldo=None, **null):
    a = {k: (None if null.get(k) else vp(k)) for k in ("rowptr", "eid", "val", "src", "A", "X", "out")}
    return _lib.load().gode_edge_matvec_f32_fwd(a["rowptr"], a["eid"], a["val"], a["src"], a["A"], a["X"], h if ldx is None else ldx,
                                                h, n_rows, a["out"], h if ldo is None else ldo, None)


def msg(h=16, n_edges=4, ldx=None, **null):
    a = {k: (None if null.get(k) else vp(k)) for k in ("src", "A", "X", "msg")}
    return _lib.load().gode_edge_matvec_msg_f32(a["src"], a["A"], a["X"], h if ldx is None else ldx, h, n_edges, a["msg"], None)


def bwd(h=16, n_edges=4, ldx=None, ldm=None, **null):
    a = {k: (None if null.get(k) else vp(k)) for k in ("edge_row", "edge_val", "src", "A", "X", "dM", "dA", "dxe")}
    return _lib.load().gode_edge_matvec_f32_bwd(a["edge_row"], a["edge_val"], a["src"], a["A"], a["X"], h if ldx is None else ldx,
                                                a["dM"], h if ldm is None else ldm, h, n_edges, a["dA"], a["dxe"], None)


def term_arrays(n, null_at=None):
    arrs = (ctypes.c_void_p * max(n, 1))(), (ctypes.c_void_p * max(n, 1))()
    for t in range(n):
        arrs[0][t], arrs[1][t] = P["t0"] + 64 * t, P["t1"] + 64 * t
    if null_at is not None:
        arrs[null_at[0]][null_at[1]] = None
    return arrs


def outer(h=16, n_terms=3, n_edges=4, ldx=None, ldm=None, null_term=None, **null):
    a = {k: (None if null.get(k) else vp(k)) for k in ("edge_row", "edge_val", "src", "dA")}
    dms, xs = term_arrays(n_terms, null_term)
    return _lib.load().gode_edge_outer_sum_f32(a["edge_row"], a["edge_val"], a["src"], n_terms, None if null.get("dM") else dms,
                                               None if null.get("X") else xs, h if ldx is None else ldx, h if ldm is None else ldm,
                                               h, n_edges, a["dA"], None)


def outer_acc(h=16, n_terms=3, n_edges=4, accumulate=1, null_term=None, **null):
    a = {k: (None if null.get(k) else vp(k)) for k in ("edge_row", "edge_val", "src", "dA")}
    dms, xs = term_arrays(n_terms, null_term)
    ws = (ctypes.c_float * max(n_terms, 1))()
    return _lib.load().gode_edge_outer_sum_acc_f32(a["edge_row"], a["edge_val"], a["src"], n_terms, None if null.get("dM") else dms,
                                                   None if null.get("X") else xs, None if null.get("w") else ws, h, n_edges,
                                                   accumulate, a["dA"], None)


def feval(save, h=16, n_rows=4, pre=None, out="out", k="k", **null):
    a = {n: (None if null.get(n) else vp(n)) for n in ("rowptr", "eid", "val", "src", "A", "S", "bias")}
    lib = _lib.load()
    head = (a["rowptr"], a["eid"], a["val"], a["src"], a["A"], a["S"], h, n_rows, a["bias"], None if pre is None else ctypes.byref(pre), 0.5, vp(out))
    return lib.gode_edge_ode_feval_save_f32(*head, vp(k), None) if save else lib.gode_edge_ode_feval_f32(*head, None)


def vjp(by_source, h=16, n_rows=4, n_edges=6, cot="default", **null):
    a = {n: (None if null.get(n) else vp(n)) for n in ("ms_rowptr", "ms_eid", "edge_row", "edge_val", "A", "fout", "dM", "dS", "dxe")}
    if not by_source:
        a["ms_rowptr"] = a["ms_eid"] = a["dS"] = None
    else:
        a["dxe"] = None
    lc = lincomb(2) if cot == "default" else cot
    return _lib.load().gode_edge_ode_vjp_f32(a["ms_rowptr"], a["ms_eid"], a["edge_row"], a["edge_val"], a["A"],
                                             None if lc is None else ctypes.byref(lc), 1.0, a["fout"], h, n_rows, n_edges, a["dM"], a["dS"],
                                             a["dxe"], None)


def test_edge_matvec_host_checks():
    for f in (fwd, msg, bwd):
        assert f(h=D.MSG_HMAX + 1) == D.E_RANGE
        assert f(h=0) == D.E_SHAPE and f(h=-1) == D.E_SHAPE and f(h=73, ldx=72) == D.E_SHAPE
    assert fwd(h=73, ldo=72) == D.E_SHAPE and bwd(h=73, ldm=72) == D.E_SHAPE
    assert fwd(n_rows=-1) == D.E_SHAPE and msg(n_edges=-1) == D.E_SHAPE and bwd(n_edges=-1) == D.E_SHAPE
    for name in ("rowptr", "src", "A", "X", "out"):              # eid and val are optional: the GPU cases run without them
        assert fwd(**{name: True}) == D.E_NULLPTR, name
    for name in ("src", "A", "X", "msg"):
        assert msg(**{name: True}) == D.E_NULLPTR, name
    for name in ("edge_row", "src", "A", "X", "dM"):             # edge_val, dA and dxe are optional
        assert bwd(**{name: True}) == D.E_NULLPTR, name
    everything = {k: True for k in NAMES}
    assert fwd(n_rows=0, **everything) == 0 and msg(n_edges=0, **everything) == 0 and bwd(n_edges=0, **everything) == 0


def test_edge_outer_sum_host_checks():
    for f in (outer, outer_acc):
        assert f(h=D.OUTER_HMAX + 1) == D.E_RANGE
        assert f(n_terms=0) == D.E_RANGE and f(n_terms=D.MAX_TERMS + 1) == D.E_RANGE and f(n_terms=-1) == D.E_RANGE
        assert f(h=0) == D.E_SHAPE and f(n_edges=-1) == D.E_SHAPE
        for name in ("edge_row", "src", "dM", "X", "dA"):        # edge_val is optional
            assert f(**{name: True}) == D.E_NULLPTR, name
        assert f(null_term=(0, 2)) == D.E_NULLPTR and f(null_term=(1, 0)) == D.E_NULLPTR
        assert f(n_edges=0, **{k: True for k in NAMES}) == 0
    assert outer(h=73, ldx=72) == D.E_SHAPE and outer(h=73, ldm=72) == D.E_SHAPE
    assert outer_acc(w=True) == D.E_NULLPTR


def test_edge_ode_host_checks():
    lib = _lib.load()
    assert lib.gode_edge_ode_supported(D.ODE_HMAX) == 1 and lib.gode_edge_ode_supported(D.ODE_HMAX + 1) == 0
    assert lib.gode_edge_ode_supported(0) == 0 and lib.gode_edge_ode_supported(1) == 1 and lib.gode_edge_ode_supported(-1) == 0
    everything = {k: True for k in NAMES}
    for save in (False, True):
        assert feval(save, h=D.ODE_HMAX + 1) == D.E_RANGE and feval(save, h=0) == D.E_SHAPE and feval(save, n_rows=-1) == D.E_SHAPE
        assert feval(save, pre=lincomb(D.MAX_TERMS + 1)) == D.E_RANGE and feval(save, pre=lincomb(-1)) == D.E_RANGE
        assert feval(save, pre=lincomb(3, null_at=1)) == D.E_NULLPTR
        for name in ("rowptr", "src", "A", "S", "bias"):         # eid and val are optional
            assert feval(save, **{name: True}) == D.E_NULLPTR, name
        assert feval(save, n_rows=0, **everything) == 0 and feval(save, n_rows=0, pre=lincomb(0), **everything) == 0
    pre = lincomb(3)
    pre.ptr[2] = P["k"]
    assert feval(True, k="out") == D.E_SHAPE and feval(True, pre=pre) == D.E_SHAPE
    for by_source in (True, False):
        assert vjp(by_source, h=D.ODE_HMAX + 1) == D.E_RANGE and vjp(by_source, h=0) == D.E_SHAPE
        assert vjp(by_source, n_rows=-1) == D.E_SHAPE and vjp(by_source, n_edges=-1) == D.E_SHAPE
        assert vjp(by_source, cot=lincomb(D.MAX_TERMS + 1)) == D.E_RANGE and vjp(by_source, cot=lincomb(0)) == D.E_RANGE
        assert vjp(by_source, cot=None) == D.E_NULLPTR and vjp(by_source, cot=lincomb(3, null_at=0)) == D.E_NULLPTR
        for name in ("fout", "dM", "edge_row", "A", "dS" if by_source else "dxe"):      # ms_eid and edge_val are optional
            assert vjp(by_source, **{name: True}) == D.E_NULLPTR, name
        assert vjp(by_source, n_rows=0, n_edges=0, **everything) == 0


# ---- sensitivity: altered copies of the restatement under the GPU tests' two comparisons ------------------------------------
def rejected(family, name, fault):
    """(keys torch.equal rejects on the exact data, keys the tolerance rejects on the real data)."""
    case = D.BY_NAME[family, name]
    out = []
    for kind in ("exact", "real"):
        d = D.inputs(case, kind)
        ref, alt = D.reference(case, d), D.reference(case, d, fault=fault)
        out.append(D.unequal(alt, ref) if kind == "exact" else D.failures(D.errors(alt, ref)))
    return out


def both(family, name, fault, *keys):
    exact, real = rejected(family, name, fault)
    assert set(keys) <= set(exact) and set(keys) <= set(real), (family, name, fault, exact, real)


def neither(family, name, fault):
    assert rejected(family, name, fault) == [[], []], (family, name, fault)


def test_dropped_257th_edge_of_a_target_is_rejected():
    both("matvec", "indeg_h16", "drop_edge_257", "out")
    both("matvec", "indeg_h91", "drop_edge_257", "out")
    both("feval", "indeg_h16", "drop_edge_257", "out", "k")
    both("feval", "indeg_h65", "drop_edge_257", "out", "k")
    neither("matvec", "width16", "drop_edge_257")                 # no target that long: the in-degree batch is needed
    neither("feval", "width16", "drop_edge_257")


def test_dropped_last_row_of_the_last_tile_is_rejected():
    both("matvec", "width91", "drop_last_row_of_last_tile", "out", "msg")
    both("matvec", "wide4096", "drop_last_row_of_last_tile", "out", "msg")
    neither("matvec", "width90", "drop_last_row_of_last_tile")    # one tile


def test_column_left_out_of_the_dot_is_rejected():
    for name in ("width1", "width8", "width9", "width73", "width257", "wide2457"):
        both("matvec", name, "skip_last_column", "out", "msg")
    for name in ("width1", "width4", "width5", "width33", "width112"):
        both("feval", name, "skip_last_column", "out", "k")


def test_ignored_edge_value_is_rejected():
    both("matvec", "width16", "ignore_edge_value", "out", "dA", "dxe")
    both("feval", "width16", "ignore_edge_value", "out", "k")
    both("vjp", "width16", "ignore_edge_value", "dS", "dxe")
    both("outer", "terms3_h73", "ignore_edge_value", "plain", "over", "acc")
    neither("matvec", "valnull_h16", "ignore_edge_value")         # the values are ones there


def test_gather_at_the_target_is_rejected():
    both("matvec", "width17", "gather_at_target", "out", "msg")
    both("feval", "width5", "gather_at_target", "out", "k")


def test_greater_or_equal_in_the_cotangent_mask_is_rejected():
    for name in ("width1", "width16", "width65", "outdeg_h33"):
        both("vjp", name, "mask_ge", "dM", "dS", "dxe")


def test_dropped_17th_edge_of_a_source_is_rejected():
    for name in ("outdeg_h16", "outdeg_h65", "eidnull_h16"):
        both("vjp", name, "drop_edge_17", "dS")
    neither("vjp", "width16", "drop_edge_17")                     # no source with that many edges


def test_dropped_last_term_of_an_outer_sum_is_rejected():
    both("outer", "terms1_h73", "drop_last_term", "plain", "over", "acc")
    both("outer", "terms8_h73", "drop_last_term", "plain", "over", "acc")
    both("outer", "terms8_h769", "drop_last_term", "plain", "over", "acc")


def test_ignored_accumulate_is_rejected():
    for name in ("terms3_h73", "terms2_h1", "terms8_h1024"):
        exact, real = rejected("outer", name, "ignore_accumulate")
        assert exact == ["acc"] and real == ["acc"], name
