"""The dispatch table of the one-head edge-attention family (csrc/edge.hip), pinned through the route queries, and the
conditions of the designed inputs that test_gpu_gat_routes.py runs the kernels on.  No GPU: the queries launch nothing and
read only the values of the pointers they are given, so the pointers here are made up.

The expected routes are written out below (maxc, PF_WIDTHS, REC_WIDTHS, expect_*), not recomputed from the library's expressions.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_routes_design as D                                           # noqa: E402

from graph_odenet_amd import _lib                                       # noqa: E402

PF, WAVE, GROUP, REC, ONE_BLOCK, TWO_STAGE = 1, 2, 3, 4, 5, 6
E_NULLPTR, E_SHAPE, E_RANGE, E_UNSUPPORTED = -1, -2, -4, -5
BELOW, ABOVE = 65_536, 65_537


def code(family, form=0):
    return family | (form << 8)


# columns per lane of the wave / lane-group / scatter kernels, written out: o <= 64 -> 1, <= 128 -> 2, <= 256 -> 4, <= 512 -> 8
def maxc(o):
    for top, m in ((64, 1), (128, 2), (256, 4), (512, 8)):
        if o <= top:
            return m
    raise AssertionError(o)


PF_WIDTHS = {4: 1, 8: 2, 16: 4, 32: 8, 64: 16}                           # o -> LPR
REC_WIDTHS = {16: 4, 32: 8, 64: 16, 128: 32, 256: 64}                    # o -> LPR


def expect_small(o):                                                     # rows <= 65 536, everything aligned
    return code(PF, PF_WIDTHS[o]) if o in PF_WIDTHS else code(WAVE, maxc(o))


def expect_large(o):                                                     # rows > 65 536, records, target-sorted, aligned
    return code(REC, REC_WIDTHS[o]) if o in REC_WIDTHS else code(GROUP, maxc(o))


def test_route_constants_are_the_headers():
    c = _lib.CONSTANTS
    assert [c["GODE_GAT_ROUTE_" + k] for k in ("PF", "WAVE", "GROUP", "REC", "ONE_BLOCK", "TWO_STAGE")] == [1, 2, 3, 4, 5, 6]
    from graph_odenet_amd import ops
    assert ops.gat_route(ops.GAT_ROUTE_REC, 16) == code(REC, 16) == 4 | 16 << 8


# ---- made-up arguments -------------------------------------------------------------------------------------------------
P = {name: 0x10000 * (k + 1) for k, name in enumerate(
    ("rowptr", "col", "val", "items", "long_rows", "partial", "src", "tgt", "ps", "pt", "as", "at", "bf", "a", "amax", "out", "w",
     "den", "dout", "dz", "da", "dpt", "dat", "c0", "c1", "c2", "scratch", "eid_s", "eid_t", "rp_s", "rp_t", "dps", "das"))}


def vp(x):
    return ctypes.c_void_p(x) if x else None


def graph(n_rows, col=False, items=True, n_long=0, partial=True, nnz=1000):
    g = _lib.Graph()
    g.rowptr, g.col, g.val = P["rowptr"], (P["col"] if col else None), P["val"]
    g.items, g.n_items = (P["items"] if items else None), n_rows + n_long
    g.long_rows, g.n_long, g.partial = (P["long_rows"] if n_long else None), n_long, (P["partial"] if partial else None)
    g.n_rows, g.nnz = n_rows, nnz
    return g


def proj(o, ps=0, pt=0, lds=0, ldt=0):
    p = _lib.GatProj()
    p.ps, p.ld_s, p.pt, p.ld_t = P["ps"] + ps, o + lds, P["pt"] + pt, o + ldt
    p.as_, p.at, p.ld_a = P["as"], P["at"], 2
    return p


def fwd(n_rows, o, out=0, bf=0, no_bf=False, g=None, act=None, launch=False, **pk):
    """act: None (NULL) or a _lib.GatAct; launch: the launching call, on arguments that stop it before any launch."""
    lib = _lib.load()
    g = g if g is not None else graph(n_rows)
    p = proj(o, **pk)
    fn = lib.gode_gat_agg_f32_fwd if launch else lib.gode_gat_agg_f32_fwd_route
    return fn(ctypes.byref(g), vp(P["src"]), vp(P["tgt"]), ctypes.byref(p), o, None if no_bf else vp(P["bf"] + bf), vp(P["a"]),
              vp(P["amax"]), 1e-9, vp(P["out"] + out), vp(P["w"]), vp(P["den"]), ctypes.byref(act) if act is not None else None, None)


def bwd(n_rows, o, terms=0, out=0, bf=0, dz=0, dout=0, term=0, dpt=True, dat=True, did=True, ld_dpt=0, no_dout=False, g=None,
        act=None, launch=False, zeroes_flag=False, **pk):
    lib = _lib.load()
    g = g if g is not None else graph(n_rows)
    p = proj(o, **pk)
    lc = _lib.LinComb()
    lc.n = terms
    for j in range(min(terms, _lib.GODE_MAX_TERMS)):
        lc.coef[j], lc.ptr[j] = 1.0, P["c%d" % min(j, 2)] + 0x100 * j + (term if j == terms - 1 else 0)
    flag = ctypes.c_int32(-7)
    fn = lib.gode_gat_agg_f32_bwd if launch else lib.gode_gat_agg_f32_bwd_route
    rt = fn(ctypes.byref(g), vp(P["src"]), vp(P["tgt"]), ctypes.byref(p), o, vp(P["bf"] + bf), vp(P["w"]), vp(P["den"]),
            vp(P["out"] + out), None if no_dout else vp(P["dout"] + dout), ctypes.byref(lc) if terms else None, -0.5,
            vp(P["dz"] + dz), vp(P["da"]), vp(P["dpt"]) if dpt else None, o + ld_dpt, vp(P["dat"]) if dat else None, 2,
            ctypes.byref(flag) if did else None, ctypes.byref(act) if act is not None else None, None)
    # the query writes nothing, nor does a launching call that the activation checks refuse; any other launching call zeroes it
    assert flag.value == (0 if zeroes_flag else -7)
    return rt


def scatter(n_rows, o, dz=0, dps=0, dpt=0, ld_s=0, ld_t=0):
    lib = _lib.load()
    return lib.gode_gat_scatter_f32_route(vp(P["rp_s"]), vp(P["eid_s"]), vp(P["rp_t"]), vp(P["eid_t"]), vp(P["dz"] + dz), vp(P["da"]),
                                          o, n_rows, vp(P["dps"] + dps), o + ld_s, vp(P["dpt"] + dpt), o + ld_t, vp(P["das"]),
                                          vp(P["dat"]), 2, None)


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_forward_routes_every_width_on_both_sides_of_the_threshold():
    for o in range(1, 513):
        assert fwd(BELOW, o) == expect_small(o), o
        assert fwd(ABOVE, o) == expect_large(o), o
        assert fwd(BELOW, o, no_bf=True) == expect_small(o), o           # an absent bias is not a misaligned one
        assert fwd(ABOVE, o, no_bf=True) == expect_large(o), o
    assert fwd(1, 16) == code(PF, 4) and fwd(1, 7) == code(WAVE, 1)


def test_backward_routes_every_width_on_both_sides_of_the_threshold():
    for o in range(1, 513):
        for terms in (0, 1, 3, 8):
            assert bwd(BELOW, o, terms) == expect_small(o), (o, terms)
            assert bwd(ABOVE, o, terms) == (expect_large(o) if o in REC_WIDTHS or terms == 0 else code(WAVE, maxc(o))), (o, terms)
    # the cotangent-combining form has no lane-group kernel: above the threshold, off the record route, it is the wave kernel
    assert bwd(ABOVE, 24, 1) == code(WAVE, 1) and bwd(ABOVE, 200, 8) == code(WAVE, 4) and bwd(ABOVE, 200, 0) == code(GROUP, 4)


BREAK_FWD = [dict(out=4), dict(bf=4), dict(ps=4), dict(pt=8), dict(lds=1), dict(ldt=2)]
BREAK_BWD = BREAK_FWD[0:1] + BREAK_FWD[2:] + [dict(dz=4), dict(dout=4)]


def test_each_alignment_condition_broken_in_turn():
    for o in PF_WIDTHS:
        for brk in BREAK_FWD:
            assert fwd(BELOW, o, **brk) == code(WAVE, 1), (o, brk)
        for brk in BREAK_BWD + [dict(bf=4)]:
            assert bwd(BELOW, o, 0, **brk) == code(WAVE, 1), (o, brk)
        for terms in (1, 3, 8):
            assert bwd(BELOW, o, terms, term=4) == code(WAVE, 1), (o, terms)
            for brk in (dict(out=4), dict(bf=4), dict(dz=8), dict(lds=3)):
                assert bwd(BELOW, o, terms, **brk) == code(WAVE, 1), (o, terms, brk)
            assert bwd(BELOW, o, terms, no_dout=True) == code(PF, PF_WIDTHS[o])  # dout may be absent when terms are given;
            assert bwd(BELOW, o, terms, dout=4) == code(WAVE, 1)                 # a misaligned one still counts (conservative)
    for o in REC_WIDTHS:
        for brk in BREAK_FWD:
            assert fwd(ABOVE, o, **brk) == code(GROUP, maxc(o)), (o, brk)
        for brk in BREAK_BWD:
            assert bwd(ABOVE, o, 0, **brk) == code(GROUP, maxc(o)), (o, brk)
        assert bwd(ABOVE, o, 0, ld_dpt=2) == code(GROUP, maxc(o))
        for terms in (1, 3, 8):
            assert bwd(ABOVE, o, terms, term=4) == code(WAVE, maxc(o)), (o, terms)
            for brk in (dict(out=4), dict(dz=8), dict(ldt=1), dict(ld_dpt=1)):
                assert bwd(ABOVE, o, terms, **brk) == code(WAVE, maxc(o)), (o, terms, brk)
        # the record backward's conditions do not look at bf (its 16-byte load then starts at a 4-byte boundary,
        # which global memory permits)
        assert bwd(ABOVE, o, 0, bf=4) == code(REC, REC_WIDTHS[o])
        assert bwd(ABOVE, o, 3, dout=4) == code(REC, REC_WIDTHS[o])              # and, with terms, not at dout, which is not read


def test_record_route_needs_its_records_its_order_and_its_outputs():
    for o in REC_WIDTHS:
        lpr, grp = REC_WIDTHS[o], code(GROUP, maxc(o))
        assert fwd(ABOVE, o, g=graph(ABOVE, col=True)) == grp                   # `col` present: edges not target-sorted
        assert bwd(ABOVE, o, g=graph(ABOVE, col=True)) == grp
        assert fwd(ABOVE, o, g=graph(ABOVE, items=False)) == grp
        assert bwd(ABOVE, o, g=graph(ABOVE, items=False)) == grp
        assert fwd(ABOVE, o, g=graph(ABOVE, n_long=3, partial=False)) == grp    # n_long > 0 without the slab
        assert bwd(ABOVE, o, g=graph(ABOVE, n_long=3, partial=False)) == grp
        assert fwd(ABOVE, o, g=graph(ABOVE, n_long=3)) == code(REC, lpr)
        assert bwd(ABOVE, o, g=graph(ABOVE, n_long=3)) == code(REC, lpr)
        assert fwd(ABOVE, o, g=graph(ABOVE, n_long=0, partial=False)) == code(REC, lpr)
        for miss in (dict(dpt=False), dict(dat=False), dict(did=False)):        # nowhere to put the target-side sums
            assert bwd(ABOVE, o, 0, **miss) == grp, (o, miss)
            assert bwd(ABOVE, o, 3, **miss) == code(WAVE, maxc(o)), (o, miss)
        assert fwd(BELOW, o, g=graph(BELOW, n_long=3)) == expect_small(o)       # records are not used at or below the threshold
        assert bwd(BELOW, o, g=graph(BELOW, n_long=3)) == expect_small(o)
    for o in PF_WIDTHS:                                                          # `col` does not matter below the threshold
        assert fwd(BELOW, o, g=graph(BELOW, col=True)) == code(PF, PF_WIDTHS[o])
        assert bwd(BELOW, o, 3, g=graph(BELOW, col=True)) == code(PF, PF_WIDTHS[o])


def test_scatter_routes():
    for n in (1, BELOW, ABOVE):                                                  # no row threshold in the scatter
        for o in range(1, 513):
            assert scatter(n, o) == (code(PF, PF_WIDTHS[o]) if o in PF_WIDTHS else code(WAVE, maxc(o))), (n, o)
    for o in PF_WIDTHS:
        for brk in (dict(dz=4), dict(dps=4), dict(dpt=8), dict(ld_s=1), dict(ld_t=2)):
            assert scatter(700, o, **brk) == code(WAVE, 1), (o, brk)


def test_validation_codes_come_back_unchanged():
    lib = _lib.load()
    assert fwd(BELOW, 513) == E_UNSUPPORTED and fwd(ABOVE, 513) == E_UNSUPPORTED
    assert bwd(BELOW, 513) == E_UNSUPPORTED and bwd(ABOVE, 513, 3) == E_UNSUPPORTED
    assert scatter(700, 513) == E_UNSUPPORTED
    assert fwd(0, 16) == 0 and bwd(0, 16) == 0 and scatter(0, 16) == 0           # nothing to launch
    assert fwd(-1, 16) == E_SHAPE and fwd(700, 0) == E_SHAPE and bwd(700, -3) == E_SHAPE and scatter(700, 0) == E_SHAPE
    assert fwd(700, 16, lds=-1) == E_SHAPE and scatter(700, 16, ld_s=-1) == E_SHAPE
    assert fwd(2 ** 31, 16) == E_RANGE and bwd(2 ** 31, 16) == E_RANGE and scatter(2 ** 31, 16) == E_RANGE
    assert bwd(700, 16, 0, no_dout=True) == E_NULLPTR
    assert bwd(700, 16, 9) == E_RANGE                                            # more than GODE_MAX_TERMS terms
    assert lib.gode_gat_agg_f32_fwd_route(None, None, None, None, 16, None, None, None, 0.0, None, None, None, None, None) == E_NULLPTR
    # and the launching calls answer the same before any launch
    assert lib.gode_gat_agg_f32_fwd(None, None, None, None, 16, None, None, None, 0.0, None, None, None, None, None) == E_NULLPTR
    g, p = graph(700), proj(513)
    assert lib.gode_gat_agg_f32_fwd(ctypes.byref(g), vp(P["src"]), vp(P["tgt"]), ctypes.byref(p), 513, None, vp(P["a"]),
                                    vp(P["amax"]), 0.0, vp(P["out"]), vp(P["w"]), vp(P["den"]), None, None) == E_UNSUPPORTED
    assert lib.gode_gat_scatter_f32(None, None, None, None, None, None, 16, 0, None, 16, None, 16, None, None, 2, None) == 0


def test_null_a_zeroed_struct_and_relu_with_the_outer_relu_are_one_spelling():
    """The `act` argument of the cases above was NULL.  A zeroed gode_gat_act_t and {RELU, nan, 1} (a parameter relu does not
    read, an outer relu that is the identity there) answer the same on every one of them: the route twin everywhere, the
    launching call wherever it returns before a launch (the pointers are made up, so nothing here may reach one)."""
    def spellings():
        return (None, _lib.GatAct(), _lib.GatAct(0, float("nan"), 1))
    f_cases = [((n, o), dict(no_bf=nb)) for o in range(1, 513) for n in (BELOW, ABOVE) for nb in (False, True)]
    b_cases = [((n, o, terms), {}) for o in range(1, 513) for n in (BELOW, ABOVE) for terms in (0, 1, 3, 8)]
    for o in PF_WIDTHS:
        f_cases += [((BELOW, o), brk) for brk in BREAK_FWD]
        b_cases += [((BELOW, o, 0), brk) for brk in BREAK_BWD + [dict(bf=4)]]
        b_cases += [((BELOW, o, 3), brk) for brk in (dict(term=4), dict(out=4), dict(dz=8), dict(no_dout=True), dict(dout=4))]
    for o in REC_WIDTHS:
        f_cases += [((ABOVE, o), brk) for brk in BREAK_FWD]
        f_cases += [((ABOVE, o), dict(g=g)) for g in (graph(ABOVE, col=True), graph(ABOVE, items=False), graph(ABOVE, n_long=3))]
        b_cases += [((ABOVE, o, 0), brk) for brk in BREAK_BWD + [dict(ld_dpt=2), dict(dpt=False), dict(dat=False), dict(did=False)]]
        b_cases += [((ABOVE, o, 3), brk) for brk in (dict(term=4), dict(ldt=1), dict(dpt=False), dict(g=graph(ABOVE, n_long=3)))]
    refused_f = [((BELOW, 513), {}), ((0, 16), {}), ((-1, 16), {}), ((700, 0), {}), ((700, 16), dict(lds=-1)), ((2 ** 31, 16), {})]
    refused_b = [((ABOVE, 513, 3), {}), ((0, 16), {}), ((700, -3), {}), ((2 ** 31, 16), {}), ((700, 16, 0), dict(no_dout=True)),
                 ((700, 16, 9), {})]
    for call, cases, refused in ((fwd, f_cases, refused_f), (bwd, b_cases, refused_b)):
        for args, kw in cases:
            codes = {call(*args, act=s, **kw) for s in spellings()}
            assert len(codes) == 1 and codes.pop() > 0, (args, kw)
        for args, kw in refused:
            twin = {call(*args, act=s, **kw) for s in spellings()}
            assert len(twin) == 1 and max(twin) <= 0, (args, kw)          # asserted BEFORE the launching call is made
            zero = dict(zeroes_flag=True) if call is bwd else {}           # the activation passed: a launching call zeroes the flag
            assert {call(*args, act=s, launch=True, **zero, **kw) for s in spellings()} == twin, (args, kw)


def test_logits_and_maxpath_thresholds():
    lib = _lib.load()
    p = proj(16)

    def logits(E, scratch=True):
        return lib.gode_gat_logits_f32_route(ctypes.byref(p), vp(P["bf"]), vp(P["src"]), vp(P["tgt"]), E, vp(P["a"]), vp(P["amax"]),
                                             vp(P["scratch"]) if scratch else None, None)

    def maxpath(E, dat=False, scratch=True):
        return lib.gode_gat_maxpath_f32_route(vp(P["a"]), vp(P["amax"]), vp(P["da"]), E, vp(P["tgt"]), vp(P["dat"]) if dat else None, 2,
                                              vp(P["scratch"]) if scratch else None, None)

    for E, want in ((0, ONE_BLOCK), (1, ONE_BLOCK), (32_768, ONE_BLOCK), (32_769, TWO_STAGE), (262_144 + 77, TWO_STAGE)):
        assert logits(E) == code(want), E
    assert logits(-1) == E_SHAPE and logits(2 ** 31) == E_RANGE and logits(5, scratch=False) == E_NULLPTR
    for E, dat, want in ((1, False, ONE_BLOCK), (32_768, False, ONE_BLOCK), (32_769, False, TWO_STAGE), (40_000, False, TWO_STAGE),
                         (1, True, TWO_STAGE), (32_768, True, TWO_STAGE), (32_769, True, TWO_STAGE)):
        assert maxpath(E, dat) == code(want), (E, dat)
    assert maxpath(0) == 0 and maxpath(-1) == E_SHAPE and maxpath(2 ** 31) == E_RANGE
    assert maxpath(100, scratch=False) == code(ONE_BLOCK)                        # one block needs no scratch
    assert maxpath(100, dat=True, scratch=False) == E_NULLPTR and maxpath(40_000, scratch=False) == E_NULLPTR


# ---- the designed inputs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["S", "L"])
def test_design_has_every_degree_slot_count_and_position(kind):
    d = D.design(kind)
    n = d.n
    assert n % 4 and n % 16
    assert (n > D.THRESHOLD) == (kind == "L")
    assert sorted(d.special.values()) == sorted(D.SHORT + D.LONG)
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(d.rows, minlength=n))
    deg = rp[1:] - rp[:-1]
    for row, s in d.special.items():
        assert deg[row] == s
        assert (row + 1 < n and deg[row + 1] == 0) or (row > 0 and deg[row - 1] == 0), row      # beside an empty row
    assert D.slot_counts(deg) == D.SLOT_COUNTS
    assert 0 in d.special and n - 1 in d.special
    bulk = np.delete(deg, list(d.special))
    assert set(bulk.tolist()) <= {0, 1, 2, 3} and {1, 2, 3} <= set(bulk.tolist())
    if kind == "L":
        assert D.THRESHOLD - 1 in d.special and D.THRESHOLD in d.special
        assert deg[D.THRESHOLD - 2] == 0 and deg[D.THRESHOLD + 1] == 0
        assert (deg[D.THRESHOLD + 2:] > 0).sum() > 300                              # work beyond the threshold row
        assert d.E < 13_000 and (deg == 0).sum() > 60_000
    for row in d.repeated:                                                           # one source node twice in a row
        assert d.src[rp[row]] == d.src[rp[row] + 1]
    assert {2, 5, 64, 193, 1000} == {d.special[r] for r in d.repeated}
    assert d.src.min() == 0 and d.src.max() == n - 1
    assert set(np.unique(d.vals).tolist()) == {0.5, 0.75, 1.0, 1.25, 1.5}
    assert D.design(kind, True, True).vals is None                                   # the pattern-only variant
    # the record list the library builds from it, split at 96
    from graph_odenet_amd.graph import CSRGraph
    g = CSRGraph(torch.from_numpy(rp), torch.arange(d.E), None, n, d.E, split=D.SPLIT)
    lr = g.long_rows.numpy()
    assert {int(x) for x in lr[:, 2] - lr[:, 1]} == D.SLOT_COUNTS and g.n_long == len([x for x in D.SHORT + D.LONG if x > D.SPLIT]) == 13
    assert g.n_items == n + sum(-(-x // D.SPLIT) - 1 for x in D.SHORT + D.LONG if x > D.SPLIT)


@pytest.mark.parametrize("kind", ["S", "L"])
def test_non_canonical_variant_disagrees_with_tgt(kind):
    d, c = D.design(kind, False), D.design(kind)
    assert d.E == c.E and np.array_equal(np.bincount(d.rows, minlength=d.n), np.bincount(c.rows, minlength=c.n))
    assert sorted(d.cols.tolist()) == list(range(d.E))                               # one entry per edge
    off = d.tgt[d.cols] != d.rows
    assert 0 < off.sum() < d.E // 5
    assert c.deg[d.rows[off]].max() <= 16                                            # long rows keep one Pt row per row
    assert (np.diff(d.cols) < 0).any()                                               # not the identity: `col` is needed
    same = d.rows[:-1] == d.rows[1:]
    assert (np.diff(d.cols)[same] > 0).all()                                         # edge-id order inside a row


@pytest.mark.parametrize("kind,canonical", [("S", True), ("L", True), ("S", False), ("L", False)])
@pytest.mark.parametrize("o", [7, 16, 128, 512])
def test_design_values_share_and_zero_fraction(kind, canonical, o):
    d, v = D.design(kind, canonical), D.values(kind, canonical, o)
    ref = D.reference(d, v)
    print("%s canonical=%s o=%d: min share %.3g, z == 0 on %.4f" % (kind, canonical, o, ref.share.min().item(),
                                                                    (ref.z == 0).double().mean().item()))
    assert ref.share.min().item() >= D.MIN_SHARE                                     # a dropped or doubled edge is >= 5 x TOL
    assert D.MIN_SHARE >= 5 * D.TOL
    assert 0.03 < (ref.z == 0).double().mean().item() < 0.06
    for x in (v.Ps, v.Pt, v.bf, v.dout, *v.cot):                                     # multiples of 1/4 in [-2, 2]
        assert x.abs().max() <= 2 and bool((x * 4 == (x * 4).round()).all())
    z32 = (v.Ps[torch.from_numpy(d.lut[d.src])] + v.Pt[torch.from_numpy(d.lut[d.tgt])]) + v.bf
    assert bool((z32.double() == ref.z).all())                                       # z is exact in fp32
    assert all(abs(cf) in (0.5, 1.0, 2.0) for cf in v.coef) and len(v.coef) == _lib.GODE_MAX_TERMS == D.MAX_TERMS
    assert {-1.0, 1.0} == {np.sign(cf) for cf in v.coef}
    assert v.bw.item() != 0 and v.A2.abs().max() <= 1


def test_reference_agrees_with_autograd_in_float64():
    """The restatement's backward against torch.autograd on its own forward (S, o = 7): an independent check of the
    formulas the GPU results are held against."""
    d, v = D.design("S", False), D.values("S", False, 7)
    ref = D.reference(d, v)
    s, t = torch.from_numpy(d.lut[d.src]), torch.from_numpy(d.lut[d.tgt])
    r, c = torch.from_numpy(d.lut[d.rows]), torch.from_numpy(d.cols)
    Ps, Pt, A2 = (x.double().requires_grad_() for x in (v.Ps, v.Pt, v.A2))
    val = torch.from_numpy(d.vals).double()
    a = (A2[s, 0] + A2[t, 1]) + v.bw.double()
    a = a + (ref.a32.double() - a).detach()                                          # the fp32 rounding of the logits, as a constant
    w = torch.exp(a - ref.amax.double())                                             # the maximum held fixed: no max path
    y = torch.relu(Ps[s] + Pt[t] + v.bf.double())
    we = val * w[c]
    na = v.Ps.shape[0]
    den = torch.zeros(na, dtype=torch.float64).index_add(0, r, we) + D.EPS
    out = torch.zeros(na, 7, dtype=torch.float64).index_add(0, r, we[:, None] * y[c]) / den[:, None]
    assert torch.allclose(out, ref.out, rtol=1e-12, atol=0)
    gPs, gPt, gA2 = torch.autograd.grad(out, (Ps, Pt, A2), v.dout.double())
    for got, want in ((gPs, ref.dPs), (gPt, ref.dPt)):
        assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    assert (gA2 - ref.dA2).abs().max().item() <= 1e-12 * ref.magA2.max().item()


def test_metric_sees_one_short_row():
    """An error confined to one one-edge row is invisible against the global maximum and plain under the row metric."""
    d, v = D.design("S"), D.values("S", True, 16)
    ref = D.reference(d, v)
    one = int(np.flatnonzero(d.deg == 1)[0])
    e = int(np.flatnonzero(d.rows == one)[0])
    bad = ref.dz.clone()
    bad[e] *= 1.001
    err, exact = D.edge_error(bad, ref.dz, ref.edge_row, v.Ps.shape[0])
    assert exact and 5e-4 < err < 2e-3
    assert (bad - ref.dz).abs().max().item() / ref.dz.abs().max().item() < err
    bad = ref.out.clone()
    bad[d.lut[one]] *= 1.001
    err, exact = D.node_error(bad, ref.out)
    assert exact and 5e-4 < err < 2e-3
    bad = ref.out.clone()
    empty = torch.nonzero(ref.out.abs().max(1).values == 0).flatten()
    assert empty.numel() > 0                                                          # rows without edges among the active nodes
    bad[empty[0], 0] = 1e-30
    assert D.node_error(bad, ref.out)[1] is False                                     # an all-zero row must be exactly zero


# ---- the comparisons bite ------------------------------------------------------------------------------------------------
# A kernel is never made wrong on a GPU to see a test fail.  Instead the arithmetic of the restatement is made wrong in the
# ways a kernel could be (gat_routes_design.FAULTS) and held against the reference with the very comparisons, inputs and
# bound of test_gpu_gat_routes.py: each fault must be rejected at the case that is there for it, by the quantity named.
def results_of(ref, bad):
    res = dict(D.compare_forward(ref, bad.w, bad.den, bad.out))
    res.update(D.compare_backward(ref, bad.dz, bad.da, bad.dPs, bad.dPt, bad.dA2))
    return res


def rejected(res):
    return sorted(q for q, (err, exact) in res.items() if not (err <= D.TOL and exact))


@pytest.mark.parametrize("fault,kind,o,terms,caught_by", [
    ("bias_first_chunk_only", "L", 73, 0, ["dA2", "da", "out"]),                      # only a width above 64 columns sees it
    ("no_val_in_backward", "L", 7, 0, ["dA2", "dPs", "dPt", "da", "dz"]),
    ("mask_ge", "L", 16, 0, ["dPs", "dPt", "dz"]),
    ("finish_one_slot_early", "L", 16, 0, ["dA2", "dPs", "dPt", "da", "den", "dz", "out"]),
    ("no_cot_scale", "S", 7, 1, ["dA2", "dPs", "dPt", "da", "dz"]),
])
def test_each_fault_is_rejected_by_the_gpu_tests_comparisons(fault, kind, o, terms, caught_by):
    d, v = D.design(kind), D.values(kind, True, o)
    ref = D.reference(d, v, terms)
    assert D.passes(results_of(ref, ref))
    res = results_of(ref, D.reference(d, v, terms, fault=fault))
    print(fault, {q: "%.2e" % e for q, (e, _) in res.items()})
    assert rejected(res) == caught_by
    assert all(res[q][0] > 50 * D.TOL for q in caught_by)                            # far beyond the bound, not by a hair


def test_bias_fault_needs_a_width_above_64_and_val_fault_needs_values():
    """Why the cases are what they are: the first is invisible at o <= 64, the second on a pattern-only matrix."""
    d, v = D.design("L"), D.values("L", True, 24)
    ref = D.reference(d, v)
    assert rejected(results_of(ref, D.reference(d, v, fault="bias_first_chunk_only"))) == []
    dp = D.design("L", True, True)
    assert rejected(results_of(D.reference(dp, v), D.reference(dp, v, fault="no_val_in_backward"))) == []
    assert rejected(results_of(ref, D.reference(d, v, fault="no_val_in_backward"))) != []


def test_finish_fault_confined_to_the_split_rows():
    """Leaving out the last slot changes only the 13 split rows - 13 of 66 003 rows, which the row metric sees in full."""
    d, v = D.design("L"), D.values("L", True, 16)
    ref, bad = D.reference(d, v), D.reference(d, v, fault="finish_one_slot_early")
    rows = torch.nonzero((ref.out - bad.out).abs().max(1).values > 0).flatten()
    assert sorted(d.act[rows.numpy()].tolist()) == sorted(r for r, s in d.special.items() if s > D.SPLIT)


def two_stage_maxpath(a, amax, da, tgt=None, dat=None, combine=min, correct_dat=True):
    """gode_gat_maxpath_f32's two-stage route restated: blocks of ceil(E / nb) edges, per block the sum and the first
    arg-max (or INT32_MAX), combined in block order."""
    E = a.numel()
    nb = max(1, min(1024, -(-E // 4096)))
    per = -(-E // nb)
    total, first = 0.0, []
    for b in range(nb):
        lo, hi = b * per, min(E, (b + 1) * per)
        total += float(da[lo:hi].double().sum())
        hit = torch.nonzero(a[lo:hi] == amax).flatten()
        first.append(lo + int(hit[0]) if hit.numel() else 2 ** 31 - 1)
    f = combine(first)
    da = da.clone()
    dat = None if dat is None else dat.clone()
    if f < E:
        da[f] -= total
        if dat is not None and correct_dat:
            dat[tgt[f]] -= total
    return da, dat


def test_maxpath_faults_are_rejected_by_the_exact_cases():
    """`max` for `min` over the blocks' candidates, and a missing dat correction, against the expectations of
    test_gpu_gat_routes.py's max-path cases (same sizes and ties)."""
    E, ties = 40_000, (13_000, 29_000, 39_999)
    rs = np.random.RandomState(E)
    a = torch.from_numpy(rs.uniform(-3, 3, E).astype(np.float32))
    a[list(ties)] = 4.0
    da = torch.from_numpy(rs.randint(-8, 9, E).astype(np.float32))
    tgt = torch.from_numpy(np.random.RandomState(E + 1).randint(0, 500, E))
    dat = torch.zeros(500).index_add_(0, tgt, da)
    S = da.double().sum().float()
    assert S.item() != 0
    want_da, want_dat = da.clone(), dat.clone()
    want_da[min(ties)] -= S
    want_dat[tgt[min(ties)]] -= S
    amax = torch.tensor(4.0)
    got_da, got_dat = two_stage_maxpath(a, amax, da, tgt, dat)
    assert torch.equal(got_da, want_da) and torch.equal(got_dat, want_dat)                 # the restatement itself is right
    bad_da, _ = two_stage_maxpath(a, amax, da, tgt, dat, combine=max)
    assert not torch.equal(bad_da, want_da)               # blocks without a tie carry INT32_MAX: no edge is corrected at all
    assert len({t // 4000 for t in ties}) == 3                                             # the ties sit in three different blocks
    _, bad_dat = two_stage_maxpath(a, amax, da, tgt, dat, correct_dat=False)
    assert not torch.equal(bad_dat, want_dat)
