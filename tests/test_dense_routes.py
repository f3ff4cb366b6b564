"""The design of the gemm.hip route tests, checked on the CPU: the limits dense_routes_design.py states are the ones in the
source, every case reaches the routes it declares (recomputed from those limits) and the tables together reach every
instantiation and loop feature of the route table, the exact data is exact (the restatement on absolute values stays below
2^24 granules and plain float32 arithmetic in four summation orders reproduces float64), every group of the real data has a
standard deviation of at least 0.5, plain float32 in four orders stays inside the derived bounds on the real data, no derived
bound is looser than the bar tests/test_gpu_kernels.py applies to the same quantity, fifteen defects planted into the float64
reference are each rejected by the comparison on every case they touch, and the entry points answer their host-side checks
through the C ABI (nothing is launched, so the pointers are made up).  No GPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_routes_design as D                                         # noqa: E402

from graph_odenet_amd import _lib                                       # noqa: E402

ID = lambda c: c.id                                                     # noqa: E731
SMALL = [c for c in D.ALL_CASES if c.n < D.LARGE_N]
# the second trips restated on the CPU: every family's once (the d = 16 term sweeps repeat one route each)
LARGE = [D.BY_ID[k] for k in ("fwd/trip2_d16_terms7", "fwd/trip2_d16_terms8", "fwd/trip2_d64", "fwd/narrow_trip2", "fwd/generic_trip2",
                              "pair/trip2", "bwd/trip2_d16_terms5", "bwd/trip2_d16_terms8", "bwd/trip2_d32", "bwd/narrow_trip2",
                              "bwd/generic_trip2", "wgrad/trip2_d16_terms6", "wgrad/trip2_d16_terms8", "wgrad/trip2_d64", "wgrad/trip2_d32_exact", "fwd/trip2_d32", "wgrad/narrow_trip2",
                              "wgrad/generic_trip2", "gn/trip2")]


# ---- limits ----------------------------------------------------------------------------------------------------------------
def test_limits_are_the_sources():
    root = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    src = open(os.path.join(root, "gemm.hip")).read()
    assert "constexpr int kMaxBlocks = %d;" % D.MAX_BLOCKS in src
    assert "constexpr int64_t kWgradSplitMinRows = %d;" % D.PC_MIN_ROWS in src
    assert "int64_t b = ((n_rows + 15) / 16 + 3) / 4;\n    if (b < 1) b = 1;\n    if (b > kMaxBlocks) b = kMaxBlocks;" in src      # fwd_blocks
    assert "int64_t b = (n_rows + 31) / 32;\n    if (b < 1) b = 1;\n    if (b > kMaxBlocks) b = kMaxBlocks;" in src                # wgrad_blocks
    assert src.count("const int n_tiles = (n_rows + 15) / 16;") == 6 and "constexpr int R = %d;                       // rows per staged tile" % D.WG_TILE in src
    assert src.count("int tile = blockIdx.x * %d + wave;" % D.WAVES) == 5 and src.count("tile += gridDim.x * %d)" % D.WAVES) == 4
    assert src.count("__launch_bounds__(256") == 9 and "for (int tile = blockIdx.x * %d + wave; tile < n_tiles; tile += gridDim.x * %d)" % (
        D.SPLIT_WAVES, D.SPLIT_WAVES) in src
    assert "constexpr int RB = %d;" % D.GEN_RB in src and src.count("if (blocks > %d) blocks = %d;" % (D.GEN_MAX_BLOCKS, D.GEN_MAX_BLOCKS)) == 2
    assert src.count("if (b > %d) b = %d; if (b < 1) b = 1;" % (D.GEN_MAX_BLOCKS, D.GEN_MAX_BLOCKS)) == 2           # gode_gemm_bwd_parts, gode_group_norm_parts
    assert "if (blocks < 1) blocks = 1; if (blocks > %d) blocks = %d;" % (D.SPLIT_MAX_BLOCKS, D.SPLIT_MAX_BLOCKS) in src
    for fn, col in (("fast_cg", "if (d_in != d_out) return -1;"), ("narrow_cg", "if (d_out != %d) return -1;" % D.NARROW_D_OUT)):
        body = src[src.index("int %s(int64_t d_in, int64_t d_out, int32_t groups) {" % fn):]
        body = body[:body.index("\n}\n")]
        assert col in body and "if (d_in != 16 && d_in != 32 && d_in != 64 && d_in != 128) return -1;" in body
        assert "if (groups == 0) return 0;" in body and "if (d_in % groups) return -1;" in body and "cg == 1 || cg == 2 || cg == 4" in body
    assert "if (n_rows > INT32_MAX || d_in > %d || d_out > %d) return GODE_E_RANGE;" % (D.MAX_D_IN, D.MAX_D_OUT) in src
    assert "if (groups > 0 && d_in % groups) return GODE_E_SHAPE;" in src
    assert "if (aux_out && !(cg >= 0 && al && d_in == %d)) return GODE_E_UNSUPPORTED;" % D.AUX_D in src
    assert "if (x_out && (((uintptr_t)x_out) & 15)) return GODE_E_ALIGN;" in src and "if (aux_out && (((uintptr_t)aux_out) & 15)) return GODE_E_ALIGN;" in src
    assert "if (aux_out == S || aux_out == x_out) return GODE_E_RANGE;" in src
    assert "if ((dgamma_part == nullptr) != (dbeta_part == nullptr)) return GODE_E_NULLPTR;" in src
    # the 16-byte conditions of the four entry points
    assert src.count("const bool al = lincomb_aligned16(xin) && !(((uintptr_t)S) & 15) && !(((uintptr_t)W) & 15) &&\n"
                     "                    (!gamma || !(((uintptr_t)gamma) & 15)) && (!beta || !(((uintptr_t)beta) & 15));") == 1
    assert ("const bool al = lincomb_aligned16(xin) && !((((uintptr_t)Sa) | ((uintptr_t)Sb) | ((uintptr_t)Wa) | ((uintptr_t)Wb)) & 15) &&\n"
            "                    (!gamma || !(((uintptr_t)gamma) & 15)) && (!beta || !(((uintptr_t)beta) & 15)) &&\n"
            "                    (!x_out || !(((uintptr_t)x_out) & 15));") in src
    assert ("const bool al = lincomb_aligned16(xin) && lincomb_aligned16(pre) && !(((uintptr_t)dS) & 15) && !(((uintptr_t)dx) & 15) &&\n"
            "                    (!gamma || !(((uintptr_t)gamma) & 15)) &&\n"
            "                    (!dgamma_part || (!(((uintptr_t)dgamma_part) & 15) && !(((uintptr_t)dbeta_part) & 15)));") in src
    assert ("const bool al = lincomb_aligned16(xin) && !(((uintptr_t)dS) & 15) &&\n"
            "                    (!gamma || !(((uintptr_t)gamma) & 15)) && (!beta || !(((uintptr_t)beta) & 15));") in src
    # the split-bf16 form and the producer / consumer forms this suite stays below
    assert ("if (cg >= 0 && al && d_in == 128 && !x_out && (gode_opt_gemm_split() == 1 || (gode_opt_gemm_split() == 2 && lc.n <= 2 && "
            "n_rows >= 65536))) {") in src
    assert src.count("(n_rows >= kWgradSplitMinRows || gode_opt_wgrad_split_small())") == 6
    assert "if (xin.n > 4) { issue_terms2<NJ>(xin, 4, nbase, nvalid, v);" in src and "if (xin.n > 6) { issue_terms2<NJ>(xin, 6, nbase, nvalid, v);" in src
    assert "if (bytes <= 64 * 1024) return 0;" in src and D.LDS_ATTR == 64 * 1024
    assert "const size_t lds = ((size_t)RB * d_in * 2 + g2 * 2) * sizeof(float);" in src
    assert "constexpr int RPP = 256 / TPR;              // rows per pass" in src
    # groups = 0: no kernel touches the partial buffers
    assert src.count("if (CG != 0 && dgamma_part) {") == 2 and "if (dgamma_part && groups > 0) {" in src
    assert _lib.GODE_MAX_TERMS == D.MAX_TERMS
    header = " ".join(open(_lib.HEADER_PATH).read().split())
    for name, value in (("NULLPTR", D.E_NULLPTR), ("SHAPE", D.E_SHAPE), ("ALIGN", D.E_ALIGN), ("RANGE", D.E_RANGE), ("UNSUPPORTED", D.E_UNSUPPORTED)):
        assert "#define GODE_E_%s (%d)" % (name, value) in header
    assert "dgamma_part and dbeta_part are left untouched where groups == 0" in header
    make = open(os.path.join(root, "Makefile")).read()
    assert "fast-math" not in make and "-Ofast" not in make and "unsafe-math" not in make


def test_limits_rederived():
    assert [D.fwd_blocks(n) for n in (0, 1, 64, 65, 32704, 32705, 32768, 10 ** 6)] == [1, 1, 1, 2, 511, 512, 512, 512]
    assert [D.wgrad_blocks(n) for n in (0, 1, 32, 33, 16384, 16385)] == [1, 1, 1, 2, 512, 512]
    assert [D.gen_blocks(n) for n in (0, 1, 8, 9, 16384, 16385)] == [1, 1, 1, 2, 2048, 2048]
    assert D.TRIP2_N == D.MAX_BLOCKS * D.WAVES * D.TILE + 21 and D.TRIP2_WG_N == D.MAX_BLOCKS * D.WG_TILE + 33 == D.GEN_MAX_BLOCKS * D.GEN_RB + 33
    assert D.TRIP2_N < D.PC_MIN_ROWS and D.TRIP2_N == D.SPLIT_MAX_BLOCKS * D.SPLIT_WAVES * D.TILE + 21
    assert D.gen_bwd_lds(2048, 0) > D.LDS_ATTR > D.gen_bwd_lds(128, 32) and D.gen_bwd_lds(2048, 0) <= 160 * 1024
    for rows, per, blocks, n in ((16, 4, D.fwd_blocks(D.TRIP2_N), D.TRIP2_N), (32, 1, D.wgrad_blocks(D.TRIP2_WG_N), D.TRIP2_WG_N), (16, 4, 1, 37), (8, 1, 2, 33)):
        parts = D.partition(rows, per, blocks, n)
        assert len(parts) == blocks and sorted(np.concatenate(parts).tolist()) == list(range(n))                 # every row once
    assert [len(p) for p in D.partition(16, 4, 512, D.TRIP2_N)[:2]] == [64 + 21, 64]                               # block 0 owns the second trip
    assert [D.fast_cg(*a) for a in ((16, 16, 16), (64, 64, 8), (128, 128, 0), (24, 24, 24), (16, 34, 16), (32, 32, 5))] == [1, -1, 0, -1, -1, -1]
    assert [D.narrow_cg(*a) for a in ((16, 2, 4), (128, 2, 0), (64, 2, 4), (16, 3, 4), (24, 2, 24))] == [4, 0, -1, -1, -1]


# ---- routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.ALL_CASES, ids=ID)
def test_every_case_reaches_its_routes(case):
    assert case.reaches and case.route() == case.reaches, (case.id, sorted(case.route() ^ case.reaches))
    assert case.n < D.PC_MIN_ROWS and case.kinds in (("exact",), ("real",))


def test_tables_reach_every_route():
    """A term-count tag counts only from a case that sees a dropped term, a loop tag (ragged tile, second trip) only from a case
    that sees a misplaced row: one or two channels per group reach those routes too, but could not tell."""
    def counted(c):
        terms = lambda t: ":terms" in t or t.endswith((":n>4", ":n>6"))                     # noqa: E731
        loop = lambda t: t.endswith((":ragged", ":trip2"))                                   # noqa: E731
        return {t for t in c.reaches if (not terms(t) or D.sees_terms(c)) and (not loop(t) or D.sees_rows(c))}
    for fam, tags in D.ROUTE_TABLE.items():
        reached = set().union(*[counted(c) for c in D.FAMILIES[fam]])
        assert reached == set(tags), (fam, sorted(reached ^ set(tags)))
    for fam, kerns in (("fwd", ("fwd", "nfwd", "gfwd", "aux")), ("bwd", ("bwd", "nbwd", "gbwd")), ("wgrad", ("wg", "nwg", "gwg"))):
        for kern in kerns:                                                                     # the 8-term arm of every kernel, seen
            assert any("%s:terms8" % kern in c.reaches and D.touches("drop_terms_5_8", c) for c in D.FAMILIES[fam]), kern
    for name in ("fwd/trip2_d32", "fwd/trip2_d64", "fwd/trip2_d128", "bwd/trip2_d32", "wgrad/trip2_d32"):
        assert D.touches("trip2_from_trip1", D.BY_ID[name]), name
    for c in D.ALL_CASES:                                                                      # no tile-edge case is blind
        if "edge_n" in c.name and c.n:
            assert D.sees_rows(c) and D.sees_terms(c), c.id
    assert len({c.id for c in D.ALL_CASES}) == len(D.ALL_CASES)
    # 16 instantiations of each of the six templates, 4 AUX, the pair launch for all 16, 12 split forms, the generic kernels
    count = lambda fam, p: len({t for t in D.ROUTE_TABLE[fam] if t.startswith(p + "<")})          # noqa: E731
    assert [count(f, p) for f, p in (("fwd", "fwd"), ("bwd", "bwd"), ("wgrad", "wg"), ("fwd", "nfwd"), ("bwd", "nbwd"), ("wgrad", "nwg"),
                                     ("fwd", "aux"), ("pair", "pair"), ("fwd", "split"))] == [16, 16, 16, 16, 16, 16, 4, 16, 12]
    every = set().union(*D.ROUTE_TABLE.values())
    assert {"gfwd:W", "gfwd:noW", "gbwd:W", "gbwd:noW", "gwg"} <= every


def test_tables_are_the_issues():
    assert (D.SWEEP_N, D.TILE_EDGES, D.WG_EDGES, D.TRIP2_N, D.TRIP2_WG_N) == (37, (1, 15, 16, 17, 63, 64, 65), (0, 31, 32, 33), 32789, 16417)
    fwd = {c.name: c for c in D.FWD_CASES}
    assert {fwd["trip2_d16_terms%d" % k].nterms for k in range(1, 9)} == set(range(1, 9))
    assert all(c.n in (D.TRIP2_N, D.TRIP2_WG_N) for c in D.ALL_CASES if c.n >= D.LARGE_N)
    assert max(c.n * max(c.d_in, c.d_out) for c in D.ALL_CASES) == 32789 * 128
    shapes = {(c.d_in, c.d_out, c.groups) for c in D.FWD_CASES if "gfwd:W" in c.reaches}
    assert shapes >= {(24, 24, 24), (40, 40, 8), (96, 96, 32), (64, 64, 8), (128, 128, 8), (16, 34, 16), (128, 258, 32), (24, 7, 0), (2048, 3, 0)}
    big = D.BY_ID["bwd/generic_2048x3"]
    assert (big.n, big.d_in, big.d_out) == (9, 2048, 3) and "gbwd:lds>64K" in big.reaches
    assert {c.mis for c in D.ALL_CASES if c.mis} == {"x0", "S", "dS", "dx"}
    assert {c.n for c in D.WGRAD_CASES if "wg<2,4>" in c.reaches} >= set(D.WG_EDGES)
    assert {c.n for c in D.FWD_CASES if "fwd<2,4>" in c.reaches} >= set(D.TILE_EDGES)
    assert {c.n for c in D.FWD_CASES if "nfwd<1,4>" in c.reaches and c.xout} >= set(D.TILE_EDGES)
    assert {c.n for c in D.BWD_CASES if "nbwd<1,4>" in c.reaches and c.npre} >= set(D.TILE_EDGES)
    assert set(D.MUTATIONS) == {m for m in D.MUTATIONS if any(D.touches(m, c) for c in SMALL + LARGE)}


# ---- data ------------------------------------------------------------------------------------------------------------------
EXACT = [c for c in SMALL + LARGE if c.kinds == ("exact",)]
REAL = [c for c in SMALL + LARGE if c.kinds == ("real",)]


@pytest.mark.parametrize("case", EXACT, ids=ID)
def test_exact_data_is_exact(case):
    """Room on the absolute values, and float32 arithmetic in four orders IS the float64 result."""
    assert D.exact_room(case) < 2.0 ** 24
    ref = D.reference(case, "exact")
    for order in D.ORDERS:
        got = D.restate(case, "exact", order)
        assert set(got) == set(ref)
        for k in ref:
            assert D.exact_equal(got[k], ref[k][0]), (case.id, order, k)
    d = D.inputs(case, "exact")
    assert 1.0 in d["coef"] and (case.nterms < 4 or 0.0 in d["coef"]) and all(abs(c) in (0, 0.25, 0.5, 1, 2, 4) for c in d["coef"])
    if case.n > 1:
        x = D.combine64(d["coef"], d["terms"])[0]
        assert len({tuple(r) for r in x[:64]}) == min(case.n, 64) and len({tuple(r) for r in x[:64].T}) == case.d_in   # rows, columns differ


@pytest.mark.parametrize("case", REAL, ids=ID)
def test_real_groups_are_spread(case):
    d = D.inputs(case, "real")
    if case.cg >= 2 and case.n:
        x = D.combine64(d["coef"], d["terms"])[0].reshape(case.n, case.groups, case.cg)
        assert x.std(2).min() >= D.MIN_STD                                                      # rstd <= 2
    if d["gamma"] is not None:
        assert 0.5 <= np.abs(d["gamma"]).min() and np.abs(d["gamma"]).max() <= 1.5 and (d["gamma"] < 0).any() and (d["gamma"] > 0).any()
    if "W" in d:
        assert np.abs(d["W"][case.has_time:]).min() >= D.W_FLOOR / np.sqrt(case.d_in) * 0.999


@pytest.mark.parametrize("case", REAL, ids=ID)
def test_real_restatements_stay_inside_the_bounds_and_the_bounds_inside_the_old_bars(case):
    ref = D.reference(case, "real")
    for order in D.ORDERS:
        got = D.restate(case, "real", order)
        assert set(got) == set(ref)
        for k, (want, bound) in ref.items():
            assert D.within(got[k], want, bound), (case.id, order, k, D.error_figures(got[k], want, bound))
    for k, (want, bound) in ref.items():
        assert float(np.max(bound, initial=0)) <= D.old_bar(case, k, want), (case.id, k, float(np.max(bound)), D.old_bar(case, k, want))


def test_comparisons_reject_nan_shape_and_one_ulp():
    ref = np.arange(1.0, 9.0)
    good = ref.astype(np.float32)
    assert D.exact_equal(good, ref) and D.within(good, ref, 0.0)
    bad = good.copy(); bad[3] = np.nan
    assert not D.exact_equal(bad, ref) and not D.within(bad, ref, np.inf)
    bad = good.copy(); bad[7] = np.nextafter(bad[7], np.float32(9))
    assert not D.exact_equal(bad, ref) and not D.within(bad, ref, 1e-7) and D.within(bad, ref, 1e-6)
    assert not D.exact_equal(good[:7], ref) and not D.within(good[:7], ref[:7].reshape(7, 1), 1.0)
    assert D.exact_equal(ref + 0.0, ref) and not D.exact_equal(np.nextafter(ref, 9.0), ref)    # a float64 sum of partials
    assert D.error_figures(good + np.float32(1), ref, 2.0) == (1.0 / 8.0, 0.5) and D.error_figures(good, ref, 0.0) == (0.0, 0.0)


# ---- planted defects ---------------------------------------------------------------------------------------------------------
def rejected(case, mut):
    kind = case.kinds[0]
    ref, got = D.reference(case, kind), D.reference(case, kind, mut)
    if kind == "exact":
        return any(not D.exact_equal(got[k][0].astype(np.float32 if k not in ("dW", "dW0") else np.float64), ref[k][0]) for k in ref)
    return any(not D.within(got[k][0], *ref[k]) for k in ref)


@pytest.mark.parametrize("mut", D.MUTATIONS)
def test_wrong_kernel_is_rejected(mut):
    """The float64 reference with one defect planted: the comparison rejects it on every case it touches, of both kinds of data."""
    touched = [c for c in SMALL + LARGE if D.touches(mut, c)]
    assert touched and {"exact", "real"} & {c.kinds[0] for c in touched}, mut
    if mut not in ("swap_gamma_beta", "neighbour_group_stats"):                                 # these two need GroupNorm
        assert {c.kinds[0] for c in touched} == {"exact", "real"}, mut
    for case in touched:
        assert rejected(case, mut), (mut, case.id)
    for case in SMALL:
        if case not in touched and case.kinds == ("exact",):
            assert not rejected(case, mut), (mut, case.id)


# ---- host-side answers: every call returns before any launch ----------------------------------------------------------------
OK = 0
P = [ctypes.c_void_p(0x10000 * (k + 1)) for k in range(12)]                 # made-up device pointers, never followed


def lc(n, base=0x100000):
    s = _lib.LinComb()
    s.n = n
    for j in range(min(max(n, 0), D.MAX_TERMS)):
        s.coef[j], s.ptr[j] = 1.0, base * (j + 1)
    return s


def test_size_functions():
    lib = _lib.load()
    for n in (0, 1, 8, 9, 37, 64, 65, 4100, 16384, 16385, D.TRIP2_WG_N, D.TRIP2_N, 10 ** 6):
        assert lib.gode_gemm_bwd_parts(n) == D.bwd_parts(n) and lib.gode_wgrad_parts(n) == D.wgrad_blocks(n)
        assert lib.gode_group_norm_parts(n) == D.gen_blocks(n)


def test_forward_host_checks():
    lib = _lib.load()
    two, ac = lc(2), (ctypes.c_float * 8)(*([1.0] * 8))
    aux = lib.gode_gn_time_gemm_xout_aux_f32
    call = lambda n=8, d=128, g=32, dout=128, S=P[0], x_out=None, coef=None, aux_out=None, W=P[1], x=two: aux(      # noqa: E731
        ctypes.byref(x), n, d, g, 1e-5, P[2], P[3], W, dout, 1, 0.5, S, x_out, coef, aux_out, None)
    assert call(n=0) == OK and call(n=0, S=None, W=None) == OK                                  # nothing to do
    assert call(n=-1) == D.E_SHAPE and call(d=0) == D.E_SHAPE and call(g=-1) == D.E_SHAPE and call(g=5) == D.E_SHAPE
    assert call(d=2049, g=0, dout=8) == D.E_RANGE and call(dout=65537) == D.E_RANGE and call(n=2 ** 31) == D.E_RANGE
    assert call(x=lc(0)) == D.E_RANGE and call(x=lc(9)) == D.E_RANGE
    assert call(S=None) == D.E_NULLPTR and call(W=None) == D.E_NULLPTR
    assert call(aux_out=P[4]) == D.E_NULLPTR                                                    # aux_out without coefficients
    assert call(x_out=ctypes.c_void_p(0x50004)) == D.E_ALIGN and call(coef=ac, aux_out=ctypes.c_void_p(0x50004)) == D.E_ALIGN
    assert call(coef=ac, aux_out=P[0]) == D.E_RANGE and call(coef=ac, aux_out=P[5], x_out=P[5]) == D.E_RANGE        # aliasing S, x_out
    assert call(coef=ac, aux_out=ctypes.c_void_p(0x200000)) == D.E_RANGE                        # ... and the second term
    assert call(d=64, g=32, dout=64, coef=ac, aux_out=P[4]) == D.E_UNSUPPORTED                  # off d = 128
    assert call(d=128, g=8, coef=ac, aux_out=P[4]) == D.E_UNSUPPORTED                           # 16 channels per group: not a fast shape
    assert call(S=ctypes.c_void_p(0x10004), coef=ac, aux_out=P[4]) == D.E_UNSUPPORTED           # a misaligned operand
    pair = lib.gode_gn_time_gemm_pair_f32
    assert pair(ctypes.byref(two), 0, 32, 16, 1e-5, P[2], P[3], None, None, 1, 0.5, None, None, None, None) == OK
    assert pair(ctypes.byref(two), 8, 32, 5, 1e-5, P[2], P[3], P[0], P[1], 1, 0.5, P[4], P[5], None, None) == D.E_SHAPE
    for hole in range(4):
        a = [None if k == hole else P[k] for k in range(4)]
        assert pair(ctypes.byref(two), 8, 32, 16, 1e-5, P[6], P[7], a[0], a[1], 1, 0.5, a[2], a[3], None, None) == D.E_NULLPTR


def test_vjp_and_weight_gradient_host_checks():
    lib = _lib.load()
    two = lc(2)
    bwd = lambda n=8, d=32, g=16, dout=32, W=P[0], dS=P[1], dx=P[2], dg=P[3], db=P[4], pre=None: lib.gode_gn_time_gemm_bwd_f32(   # noqa: E731
        ctypes.byref(two), n, d, g, 1e-5, P[5], W, dout, 1, dS, 1.0, pre, dx, dg, db, None)
    assert bwd(n=0) == OK and bwd(n=0, W=None, dS=None, dx=None, dg=P[3], db=None) == OK
    assert bwd(dg=None) == D.E_NULLPTR and bwd(db=None) == D.E_NULLPTR                          # one of the two partial buffers
    assert bwd(W=None) == D.E_NULLPTR and bwd(dS=None) == D.E_NULLPTR and bwd(dx=None) == D.E_NULLPTR
    assert bwd(g=5) == D.E_SHAPE and bwd(d=2049, g=0) == D.E_RANGE and bwd(n=-1) == D.E_SHAPE
    assert bwd(pre=ctypes.byref(lc(9))) == D.E_RANGE
    wg = lambda n=8, d=32, g=16, dout=32, dS=P[1], part=P[2]: lib.gode_wgrad_f32(ctypes.byref(two), n, d, g, 1e-5, P[5], P[6], dS, dout, 1, part, None)  # noqa: E731
    assert wg(part=None) == D.E_NULLPTR and wg(dS=None) == D.E_NULLPTR and wg(n=0, part=None) == D.E_NULLPTR       # n = 0 still writes a partial
    assert wg(g=5) == D.E_SHAPE and wg(d=2049, g=0) == D.E_RANGE and wg(n=-1) == D.E_SHAPE
    gf, gb = lib.gode_group_norm_f32_fwd, lib.gode_group_norm_f32_bwd
    assert gf(P[0], 0, 8, 2, 1e-5, None, None, P[1], None) == OK and gf(P[0], 4, 8, 0, 1e-5, None, None, P[1], None) == D.E_SHAPE
    assert gf(P[0], 4, 8, 3, 1e-5, None, None, P[1], None) == D.E_SHAPE and gf(None, 4, 8, 2, 1e-5, None, None, P[1], None) == D.E_NULLPTR
    assert gf(P[0], 4, 2052, 4, 1e-5, None, None, P[1], None) == D.E_RANGE
    assert gb(P[0], 0, 8, 2, 1e-5, None, P[1], P[2], None, None, None) == OK and gb(P[0], 4, 8, 2, 1e-5, None, P[1], P[2], P[3], None, None) == D.E_NULLPTR
    assert gb(P[0], 4, 8, 3, 1e-5, None, P[1], P[2], None, None, None) == D.E_SHAPE and gb(P[0], 4, 2052, 4, 1e-5, None, P[1], P[2], None, None, None) == D.E_RANGE
