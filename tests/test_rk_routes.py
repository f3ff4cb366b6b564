"""The design of the rk.hip route tests, checked on the CPU: the limits rk_routes_design.py states are the ones in the source,
every case reaches the routes it declares (recomputed from those limits) and the tables together reach every tag of the route
table, the exact data is exact (the restatement on absolute values stays below 2^24 granules, 2^53 for the squared ratios, and
plain float32 arithmetic in two summation orders reproduces float64), plain float32 in both orders stays inside the derived
bounds on the real data, fifteen wrong kernels restated on the CPU are each rejected by the exact comparison on every case
whose route they touch and by the real comparison on the case the design names, and the entry points answer their host-side
checks through the C ABI (nothing is launched, so the pointers are made up).  No GPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rk_routes_design as D                                            # noqa: E402

from graph_odenet_amd import _lib                                       # noqa: E402

SINGLE = [c for c in D.ALL_CASES if not hasattr(c, "comps")]
LEAVES = SINGLE + [k for c in D.ALL_CASES if hasattr(c, "comps") for k in c.comps]
ID = lambda c: c.id                                                     # noqa: E731


# ---- limits ----------------------------------------------------------------------------------------------------------------
def test_limits_are_the_sources():
    root = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    rk = open(os.path.join(root, "rk.hip")).read()
    assert "__launch_bounds__(%d)" % D.THREADS in rk and "__launch_bounds__(" not in rk.replace("__launch_bounds__(%d)" % D.THREADS, "")
    assert rk.count("dim3(256)") == rk.count("hipLaunchKernelGGL(")
    assert rk.count("if (blocks > %d) blocks = %d;" % (D.LC_MAX_BLOCKS, D.LC_MAX_BLOCKS)) == 4       # both forms, multi, gode_zero_f32
    assert "constexpr int RED_BLOCKS = %d;" % D.RED_BLOCKS in rk
    assert "int64_t b = (n + %d) / %d;\n    if (b < 1) b = 1;\n    if (b > RED_BLOCKS) b = RED_BLOCKS;" % (D.RED_PER_BLOCK - 1, D.RED_PER_BLOCK) in rk
    assert "if (n % 4 == 0 && !(((uintptr_t)out) & 15) && lincomb_aligned16(lc)) {" in rk
    assert "(ns[c] % 4 == 0 && !(((uintptr_t)outs[c]) & 15) && lincomb_aligned16(&lcs[c])) ? 1 : 0;" in rk
    assert "if (n % 4 == 0 && lincomb_aligned16(elc) && !((((uintptr_t)y0) | ((uintptr_t)y1)) & 15))" in rk
    assert "(ns[c] % 4 == 0 && lincomb_aligned16(&elcs[c]) && !((((uintptr_t)y0[c]) | ((uintptr_t)y1[c])) & 15)) ? 1 : 0;" in rk
    assert "if (n % 4 == 0 && lincomb_aligned16(lc) && !(((uintptr_t)y) & 15))" in rk
    assert "if (len >= %d && n_part >= %d && len %% 4 == 0 && !((((uintptr_t)out) | ((uintptr_t)part)) & 15)) {" % (
        D.PARTS4_MIN_LEN, D.PARTS4_MIN_PARTS) in rk
    assert rk.count("__shared__ float sm[%d][33];" % D.PARTS_GROUPS) == 3 and rk.count("for (; p + 24 < n_part; p += 32) {") == 2
    assert rk.count("for (; p < n_part; p += %d)" % D.PARTS_GROUPS) == 2
    assert "__shared__ float4 sm[%d][17];" % D.PARTS4_GROUPS in rk and "for (; p + 48 < n_part; p += 64) {" in rk
    assert "for (; p < n_part; p += %d) {" % D.PARTS4_GROUPS in rk
    assert "int64_t b = (n_rows + %d) / %d;\n    if (b < 1) b = 1;\n    if (b > %d) b = %d;" % (
        D.COLSUM_ROWS - 1, D.COLSUM_ROWS, D.COLSUM_MAX_BLOCKS, D.COLSUM_MAX_BLOCKS) in rk
    assert rk.count("const int64_t rpb = (n_rows + nb - 1) / nb;") == 2 and rk.count("rpb > 0 ? rpb : 1") == 4
    assert "if (d >= %d && n_rows <= %d * d) {" % (D.WIDE_MIN_D, D.WIDE_ROWS_PER_D) in rk
    assert rk.count("if (d %% 4 == 0 && d <= %d && !(((uintptr_t)X) & 15) && !(((uintptr_t)scratch) & 15))" % D.COLSUM4_MAX_D) == 2
    assert "if (d <= %d) {" % D.COLSUM_HALF in rk
    assert "for (; r + 56 < n_rows; r += %d) {" % D.WIDE_TRIP in rk and "for (; r < n_rows; r += %d) s += X[r * d + c];" % D.WIDE_GROUPS in rk
    assert "for (int64_t c0 = 0; c0 < g.time_len[s]; c0 += %d) {" % D.SEG_COLS in rk and "blk += (int)((q.len + 31) / 32);" in rk
    assert _lib.GODE_MAX_TERMS == D.MAX_TERMS and _lib.CONSTANTS["GODE_MAX_REDUCE_SEGS"] == D.MAX_SEGS
    header = " ".join(open(_lib.HEADER_PATH).read().split())
    for name, value in (("NULLPTR", D.E_NULLPTR), ("SHAPE", D.E_SHAPE), ("RANGE", D.E_RANGE)):
        assert "#define GODE_E_%s (%d)" % (name, value) in header
    make = open(os.path.join(root, "Makefile")).read()
    assert "fast-math" not in make and "-Ofast" not in make and "unsafe-math" not in make        # float32 division is correctly rounded


def test_limits_rederived():
    assert [D.red_blocks(n) for n in (1, 1024, 1025, 1047552, 1047553, 1 << 30)] == [1, 1, 2, 1023, 1024, 1024]
    assert D.LC_WRAP1_N == D.LC_MAX_BLOCKS * D.THREADS + 1 and D.LC_WRAP4_N == 4 * D.LC_WRAP1_N
    assert D.ERR_FULL_N == 4 * D.RED_BLOCKS * D.THREADS and D.ERR_WRAP4_N == D.ERR_FULL_N + 4 and D.ERR_WRAP1_N == D.ERR_FULL_N + 1
    assert [D.colsum_blocks(n) for n in (0, 1, 256, 257, 262144, 262145)] == [1, 1, 1, 2, 1024, 1024]
    assert D.colsum_rpb(D.COLSUM_BIG_ROWS) == 257 and 1022 * 257 >= D.COLSUM_BIG_ROWS > 1021 * 257          # two blocks start past the end
    assert D.block_rows(D.COLSUM_BIG_ROWS)[-2:] == [(D.COLSUM_BIG_ROWS, D.COLSUM_BIG_ROWS)] * 2
    assert sum(b - a for a, b in D.block_rows(D.COLSUM_BIG_ROWS)) == D.COLSUM_BIG_ROWS
    for groups in (D.PARTS_GROUPS, D.PARTS4_GROUPS):
        for n_part in range(0, 200):
            assert D.kept_parts(n_part, groups)[0] == list(range(n_part))                                 # every partial row once
    assert D.kept_parts(25, 8)[1:] == (True, True) and D.kept_parts(24, 8)[1:] == (False, True) and D.kept_parts(32, 8)[1:] == (True, False)
    assert D.kept_parts(64, 16)[1:] == (True, False) and D.kept_parts(65, 16)[1:] == (True, True) and D.kept_parts(48, 16)[1:] == (False, True)


# ---- routes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.ALL_CASES, ids=ID)
def test_every_case_reaches_its_routes(case):
    assert case.reaches and case.route() == case.reaches, (case.id, sorted(case.route() ^ case.reaches))


def test_tables_reach_every_route():
    for fam, tags in D.ROUTE_TABLE.items():
        reached = set().union(*[c.reaches for c in D.FAMILIES[fam]])
        assert reached == set(tags), (fam, sorted(reached ^ set(tags)))
    assert len({c.id for c in D.ALL_CASES}) == len(D.ALL_CASES) and len({c.id for c in LEAVES}) == len(LEAVES)


def test_tables_are_the_issues():
    assert [n for n, _ in D.LC_N] == [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1028] and (D.LC_WRAP1_N, D.LC_WRAP4_N) == (2097153, 8388612)
    assert D.BY_ID["lincomb/wrap4"].nterms == 2
    assert [n for n, _ in D.ERR_N] == [1, 3, 4, 1023, 1024, 1025, 1028, 4096]
    assert (D.ERR_FULL_N, D.ERR_WRAP4_N, D.ERR_WRAP1_N) == (1048576, 1048580, 1048577)
    assert {c.n_part for c in D.PARTS_CASES} == {0, 1, 7, 8, 9, 24, 25, 32, 33, 37, 57, 63, 64, 65, 79, 80, 81, 112, 113, 128, 512}
    assert {c.len for c in D.PARTS_CASES} == {1, 31, 32, 33, 1000, 4092, 4096, 4097, 4100}
    assert {(c.n_part, c.len) for c in D.PARTS_CASES if "parts4" in c.reaches} >= {(64, 4096), (64, 4100)}
    assert {(c.n_part, c.len, c.mis_out) for c in D.PARTS_CASES if "parts" in c.reaches} >= {(63, 4096, False), (64, 4097, False), (64, 4096, True)}
    assert {(c.n_part, c.len) for c in D.PARTS2_CASES} == {(37, 33), (9, 1)}
    segs = [s for c in D.SEGS_CASES for s in c.segs]
    assert {s["len"] for s in segs} == {1, 31, 32, 33, 300} and {s["n_part"] for s in segs} == {0, 1, 8, 9, 33}
    assert {c.d for c in D.COLSUM_CASES if "f32:colsum4" in c.reaches} == {4, 12, 128, 300, 512, 1024}
    assert {c.d for c in D.COLSUM_CASES if "f32:colsum<=256" in c.reaches} == {1, 3, 7, 12, 73, 255, 256}
    assert {(c.n_rows, c.d) for c in D.COLSUM_CASES if "f32:colsum>256" in c.reaches} == {(513, 257), (257, 301), (255, 511), (2053, 513), (4113, 1028)}
    wide = {(c.n_rows, c.d) for c in D.COLSUM_CASES if "f32:wide" in c.reaches}
    assert wide == {(2048, 512)} | {(n, d) for n in (0, 1, 7, 8, 9, 63, 64, 65, 127, 128) for d in (513, 2667)}
    assert {c.n_rows for c in D.COLSUM_CASES if "f32:wide" not in c.reaches} >= {0, 1, 2, 255, 256, 257, 513, 262400}
    large = [c for c in LEAVES if getattr(c, "n", 0) >= D.LARGE_N]
    assert {c.n for c in large} == {D.LC_WRAP1_N, D.LC_WRAP4_N, D.ERR_FULL_N, D.ERR_WRAP4_N, D.ERR_WRAP1_N}     # the smallest sizes that wrap
    assert set(D.MUTATION_REAL_CASE) == set(D.MUTATIONS) and all(v in D.BY_ID for v in D.MUTATION_REAL_CASE.values())


# ---- data ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LEAVES, ids=ID)
def test_exact_data_is_exact(case):
    """Room on the absolute values, and float32 arithmetic in two orders IS the float64 result."""
    assert D.exact_room(case) < (2.0 ** 53 if case.family == "err" else 2.0 ** 24)
    ref = D.reference(case, "exact")
    for order in ("seq", "pair"):
        got = D.restate(case, "exact", order)
        assert set(got) == set(ref)
        for k in ref:
            assert D.exact_equal(got[k], ref[k][0]), (case.id, order, k)
    if case.family == "err":
        d = D.inputs(case, "exact")
        if case.plant is None and case.n >= 1023:
            bigger = float(np.mean(np.abs(d["y1"]) > np.abs(d["y0"])))
            assert 0.4 < bigger < 0.6 and not np.any(np.abs(d["y1"]) == np.abs(d["y0"]))
        if case.plant is not None:
            r = D.err_terms(case, d)[0]
            assert np.count_nonzero(r) == 1 and r[case.plant] != 0 and ref["sum"][0] == r[case.plant] ** 2      # exactly that one ratio squared


@pytest.mark.parametrize("case", LEAVES, ids=ID)
def test_real_restatements_stay_inside_the_bounds(case):
    ref = D.reference(case, "real")
    for order in ("seq", "pair"):
        got = D.restate(case, "real", order)
        for k, (want, bound) in ref.items():
            assert D.within(got[k], want, bound), (case.id, order, k, D.error_figures(got[k], want, bound))


def test_comparisons_reject_nan_shape_and_one_ulp():
    ref = np.arange(1.0, 9.0)
    good = ref.astype(np.float32)
    assert D.exact_equal(good, ref) and D.within(good, ref, 0.0)
    bad = good.copy(); bad[3] = np.nan
    assert not D.exact_equal(bad, ref) and not D.within(bad, ref, np.inf)
    bad = good.copy(); bad[7] = np.nextafter(bad[7], np.float32(9))
    assert not D.exact_equal(bad, ref) and not D.within(bad, ref, 1e-7) and D.within(bad, ref, 1e-6)
    assert not D.exact_equal(good[:7], ref) and not D.within(good[:7], ref[:7].reshape(7, 1), 1.0)
    assert D.exact_equal(4.0, 4.0) and not D.exact_equal(np.nextafter(4.0, 5.0), 4.0) and not D.within(float("nan"), 4.0, np.inf)
    assert D.error_figures(good + np.float32(1), ref, 2.0) == (1.0 / 8.0, 0.5) and D.error_figures(good, ref, 0.0) == (0.0, 0.0)


# ---- wrong kernels -----------------------------------------------------------------------------------------------------------
def rejected(case, kind, mut):
    ref = D.reference(case, kind)
    got = D.restate(case, kind, "seq", mut)
    if kind == "exact":
        return any(not D.exact_equal(got[k], ref[k][0]) for k in ref)
    return any(not D.within(got[k], *ref[k]) for k in ref)


@pytest.mark.parametrize("mut", D.MUTATIONS)
def test_wrong_kernel_is_rejected(mut):
    """`mut` restated on the CPU: the exact comparison rejects it on every case whose route it touches (and on no other), the
    real comparison on the case the design names."""
    touched = [c for c in LEAVES if D.touches(mut, c)]
    assert touched, mut
    for case in touched:
        assert rejected(case, "exact", mut), (mut, case.id)
    for case in LEAVES:
        if case not in touched and getattr(case, "n", 0) < D.LARGE_N and getattr(case, "n_rows", 0) < D.LARGE_N // 4:
            assert not rejected(case, "exact", mut), (mut, case.id)
    named = D.BY_ID[D.MUTATION_REAL_CASE[mut]]
    assert D.touches(mut, named) and rejected(named, "real", mut), (mut, named.id)


# ---- host-side answers: every call returns before any launch ----------------------------------------------------------------
OK, NULLPTR, SHAPE, RANGE = 0, D.E_NULLPTR, D.E_SHAPE, D.E_RANGE
P = [ctypes.c_void_p(0x10000 * (k + 1)) for k in range(12)]                 # made-up device pointers, never followed


def lc(n, null_at=None):
    s = _lib.LinComb()
    s.n = n
    for j in range(min(max(n, 0), D.MAX_TERMS)):
        s.coef[j], s.ptr[j] = 1.0, (None if j == null_at else 0x100000 * (j + 1))
    return s


def arr(ctype, values):
    return (ctype * len(values))(*values)


def test_lincomb_host_checks():
    lib = _lib.load()
    one = lc(1)
    assert lib.gode_lincomb_f32(None, None, 0, None) == OK                                   # nothing to do, nothing looked at
    assert lib.gode_lincomb_f32(None, ctypes.byref(one), 4, None) == NULLPTR
    assert lib.gode_lincomb_f32(P[0], None, 4, None) == NULLPTR
    assert lib.gode_lincomb_f32(P[0], ctypes.byref(lc(0)), 4, None) == RANGE
    assert lib.gode_lincomb_f32(P[0], ctypes.byref(lc(9)), 4, None) == RANGE
    assert lib.gode_lincomb_f32(P[0], ctypes.byref(lc(-1)), 4, None) == RANGE
    assert lib.gode_lincomb_f32(P[0], ctypes.byref(lc(8, null_at=7)), 4, None) == NULLPTR
    assert lib.gode_lincomb_f32(P[0], ctypes.byref(lc(9)), -4, None) == SHAPE                # the size first
    outs, lcs, ns = arr(ctypes.c_void_p, [0x1000, 0x2000]), (_lib.LinComb * 2)(lc(2), lc(3)), arr(ctypes.c_int64, [4, 5])
    multi = lib.gode_lincomb_multi_f32
    assert multi(None, lcs, ns, 2, None) == NULLPTR and multi(outs, None, ns, 2, None) == NULLPTR and multi(outs, lcs, None, 2, None) == NULLPTR
    assert multi(outs, lcs, ns, 0, None) == RANGE and multi(outs, lcs, ns, 5, None) == RANGE and multi(outs, lcs, ns, -1, None) == RANGE
    assert multi(outs, lcs, arr(ctypes.c_int64, [4, -1]), 2, None) == SHAPE
    assert multi(outs, lcs, arr(ctypes.c_int64, [0, 0]), 2, None) == OK                      # every component empty: no launch
    assert multi(arr(ctypes.c_void_p, [None, None]), (_lib.LinComb * 2)(lc(0), lc(9)), arr(ctypes.c_int64, [0, 0]), 2, None) == OK
    assert multi(arr(ctypes.c_void_p, [0x1000, None]), lcs, ns, 2, None) == NULLPTR
    assert multi(arr(ctypes.c_void_p, [0x1000, None]), lcs, arr(ctypes.c_int64, [0, 5]), 2, None) == NULLPTR
    assert multi(outs, (_lib.LinComb * 2)(lc(2), lc(0)), ns, 2, None) == RANGE
    assert multi(outs, (_lib.LinComb * 2)(lc(2), lc(9)), ns, 2, None) == RANGE
    assert multi(outs, (_lib.LinComb * 2)(lc(2, null_at=1), lc(3)), ns, 2, None) == NULLPTR


def test_error_sum_host_checks():
    lib = _lib.load()
    assert lib.gode_rk_errnorm_scratch_bytes() == 4 * D.RED_BLOCKS * 8
    three = lc(3)
    err, ssq = lib.gode_rk_errnorm_f32, lib.gode_rk_scaled_sumsq_f32
    for n in (0, -1):
        assert err(P[0], P[1], P[2], ctypes.byref(three), 1e-3, 1e-4, n, P[3], None) == SHAPE
        assert ssq(P[0], ctypes.byref(three), P[1], 1e-3, 1e-4, n, P[3], None) == SHAPE
    for hole in range(4):
        a = [None if k == hole else P[k] for k in range(4)]
        assert err(a[0], a[1], a[2], ctypes.byref(three), 1e-3, 1e-4, 8, a[3], None) == NULLPTR
    for hole in range(3):
        a = [None if k == hole else P[k] for k in range(3)]
        assert ssq(a[0], ctypes.byref(three), a[1], 1e-3, 1e-4, 8, a[2], None) == NULLPTR
    for bad, code in ((None, NULLPTR), (lc(0), RANGE), (lc(9), RANGE), (lc(3, null_at=0), NULLPTR)):
        ref = None if bad is None else ctypes.byref(bad)
        assert err(P[0], P[1], P[2], ref, 1e-3, 1e-4, 8, P[3], None) == code
        assert ssq(P[0], ref, P[1], 1e-3, 1e-4, 8, P[3], None) == code
    multi = lib.gode_rk_errnorm_multi_f32
    y0, y1, lcs, ns = arr(ctypes.c_void_p, [0x1000, 0x2000]), arr(ctypes.c_void_p, [0x3000, 0x4000]), (_lib.LinComb * 2)(lc(2), lc(3)), arr(ctypes.c_int64, [4, 5])
    full = [P[0], y0, y1, lcs, ns, 2, 1e-3, 1e-4, P[1], None]
    for hole in (0, 1, 2, 3, 4, 8):
        assert multi(*[None if k == hole else v for k, v in enumerate(full)]) == NULLPTR
    for count in (0, 5, -1):
        assert multi(P[0], y0, y1, lcs, ns, count, 1e-3, 1e-4, P[1], None) == RANGE
    for n1 in (0, -1):                                                                       # unlike the combine, an empty component is refused
        assert multi(P[0], y0, y1, lcs, arr(ctypes.c_int64, [4, n1]), 2, 1e-3, 1e-4, P[1], None) == SHAPE
    assert multi(P[0], arr(ctypes.c_void_p, [0x1000, None]), y1, lcs, ns, 2, 1e-3, 1e-4, P[1], None) == NULLPTR
    assert multi(P[0], y0, arr(ctypes.c_void_p, [None, 0x4000]), lcs, ns, 2, 1e-3, 1e-4, P[1], None) == NULLPTR
    assert multi(P[0], y0, y1, (_lib.LinComb * 2)(lc(2), lc(0)), ns, 2, 1e-3, 1e-4, P[1], None) == RANGE
    assert multi(P[0], y0, y1, (_lib.LinComb * 2)(lc(9), lc(3)), ns, 2, 1e-3, 1e-4, P[1], None) == RANGE
    assert multi(P[0], y0, y1, (_lib.LinComb * 2)(lc(2), lc(3, null_at=2)), ns, 2, 1e-3, 1e-4, P[1], None) == NULLPTR


def test_reduce_parts_host_checks():
    lib = _lib.load()
    one, two = lib.gode_reduce_parts_f32, lib.gode_reduce_parts2_f32
    assert one(P[0], P[1], -1, 8, 1.0, 0, None) == SHAPE and one(P[0], P[1], 4, -1, 1.0, 0, None) == SHAPE
    assert one(None, None, 4, 0, 1.0, 0, None) == OK                                         # nothing to write
    assert one(None, P[1], 4, 8, 1.0, 0, None) == NULLPTR and one(P[0], None, 4, 8, 1.0, 0, None) == NULLPTR
    assert one(None, None, 0, 8, 1.0, 0, None) == NULLPTR                                    # no partials: out is still written
    assert two(P[0], P[1], P[2], P[3], -1, 8, 1.0, 0, None) == SHAPE and two(P[0], P[1], P[2], P[3], 4, -1, 1.0, 0, None) == SHAPE
    assert two(None, None, None, None, 4, 0, 1.0, 0, None) == OK
    for hole in range(4):
        a = [None if k == hole else P[k] for k in range(4)]
        assert two(a[0], a[1], a[2], a[3], 4, 8, 1.0, 0, None) == NULLPTR
    assert two(None, None, P[2], None, 0, 8, 1.0, 0, None) == NULLPTR and two(P[0], None, None, None, 0, 8, 1.0, 0, None) == NULLPTR


def seg(**kw):
    s = _lib.ReduceSeg()
    f = dict(out=0x1000, part=0x2000, n_part=4, ld=8, col0=0, col_stride=1, len=8, w_row0=None, time_len=0)
    f.update(kw)
    for k, v in f.items():
        setattr(s, k, v)
    return s


def test_reduce_segments_host_checks():
    lib = _lib.load()
    call = lambda segs, n=None, at=P[0]: lib.gode_reduce_segments_f32((_lib.ReduceSeg * max(len(segs), 1))(*segs), len(segs) if n is None else n, 0.5, at, None)  # noqa: E731
    assert lib.gode_reduce_segments_f32(None, 1, 0.5, P[0], None) == NULLPTR
    assert call([seg()], n=0) == RANGE and call([seg()] * 9) == RANGE and call([seg()], n=-1) == RANGE
    assert call([seg(out=None)]) == NULLPTR and call([seg(part=None)]) == NULLPTR
    assert call([seg(len=0)]) == SHAPE and call([seg(len=-1)]) == SHAPE and call([seg(n_part=-1)]) == SHAPE
    assert call([seg(col_stride=0)]) == SHAPE and call([seg(col_stride=-1)]) == SHAPE and call([seg(col0=-1)]) == SHAPE
    assert call([seg(ld=7)]) == SHAPE                                                        # ld < col0 + (len - 1) * col_stride + 1
    assert call([seg(col0=1)]) == SHAPE and call([seg(col_stride=2, ld=14)]) == SHAPE and call([seg(col0=2, col_stride=3, ld=23)]) == SHAPE
    big = (2 ** 31 - 1) * 16 + 1
    assert call([seg(len=big, ld=big)]) == RANGE
    assert call([seg(w_row0=0x3000, time_len=9)]) == SHAPE                                   # time_len > len
    assert call([seg(w_row0=0x3000, time_len=9)], at=None) == SHAPE
    assert call([seg(w_row0=0x3000, time_len=8)], at=None) == NULLPTR                        # a time segment without at
    assert call([seg(), seg(w_row0=0x3000, time_len=1)], at=None) == NULLPTR
    assert call([seg(), seg(len=0)]) == SHAPE                                                # the second segment is checked as the first


def test_colsum_host_checks():
    lib = _lib.load()
    full, parts, n_parts = lib.gode_colsum_f32, lib.gode_colsum_parts_f32, ctypes.c_int64(-7)
    np_ref = ctypes.cast(ctypes.byref(n_parts), ctypes.c_void_p)
    for n_rows, d in ((-1, 8), (4, 0), (4, -1), (0, 0)):
        assert full(P[0], P[1], n_rows, d, 1.0, 0, P[2], None) == SHAPE
        assert parts(P[1], n_rows, d, P[2], np_ref, None) == SHAPE
    assert full(None, P[1], 4, 8, 1.0, 0, P[2], None) == NULLPTR and full(P[0], P[1], 4, 8, 1.0, 0, None, None) == NULLPTR
    assert full(P[0], None, 4, 8, 1.0, 0, P[2], None) == NULLPTR
    assert parts(P[1], 4, 8, None, np_ref, None) == NULLPTR and parts(P[1], 4, 8, P[2], None, None) == NULLPTR
    assert parts(None, 4, 8, P[2], np_ref, None) == NULLPTR
    assert full(P[0], P[1], 4, 2 ** 31, 1.0, 0, P[2], None) == RANGE and parts(P[1], 4, 2 ** 31, P[2], np_ref, None) == RANGE
    assert n_parts.value == -7                                                               # a refused call leaves it alone
    size = lib.gode_colsum_scratch_bytes
    assert [size(n, 5) for n in (0, 1, 256, 257)] == [20, 20, 20, 40]
    cap = D.COLSUM_MAX_BLOCKS * D.COLSUM_ROWS
    assert [size(n, 3) for n in (cap - 256, cap - 255, cap, cap + 1, 10 ** 12)] == [1023 * 12, 1024 * 12, 1024 * 12, 1024 * 12, 1024 * 12]
    assert size(D.COLSUM_BIG_ROWS, 4) == D.COLSUM_MAX_BLOCKS * 16 and size(10, 2 ** 31) == 2 ** 33
