"""Designed inputs, the float64 reference and the derived bounds for the route tests of csrc/rk.hip (test_rk_routes.py checks
the design's conditions on the CPU, test_gpu_rk_routes.py runs the kernels on it).  numpy only; nothing of the library and
nothing of oracle/ is used here.

Entry points covered: gode_lincomb_f32, gode_lincomb_multi_f32, gode_rk_errnorm_f32, gode_rk_errnorm_multi_f32,
gode_rk_scaled_sumsq_f32, gode_reduce_parts_f32, gode_reduce_parts2_f32, gode_reduce_segments_f32, gode_colsum_f32,
gode_colsum_parts_f32 and the scratch-size functions.  The limits their routes branch on are written out below as plain
numbers (test_rk_routes.py asserts them textually against rk.hip); every case declares the routes it is meant to reach as
literals, and `route(case)` recomputes them from the numbers.

Two kinds of data per case.

`exact`.  Combines and sums: integers of magnitude 1 .. 8 (matrices: one sign per column, so that no subset of a column's
addends cancels; vectors: a random sign per element), coefficients and scales powers of two (an exact 1.0 and a 0.0 among the
coefficients).  Every partial sum in any order is a multiple of the case's granularity below 2^24 times it (exact_room: the
restatement on absolute values), so float32 reproduces the float64 result bit for bit, with or without a fused multiply-add.
Error sums: rtol = 0.5, atol = 0.25, |y0| and |y1| from {0.5, 1.5, 3.5, 7.5} (never equal at one element: |y1| > |y0| at about
half of them) with random signs, so the tolerance is exactly 0.5, 1, 2 or 4; the error combination is a multiple of 4 below
2^10 (terms of magnitude 1 .. 8, coefficients +-4 and +-8), so every ratio is an integer, every square exact and the sum below
2^53: the comparison is == on the float64 sum.  (rtol = 0 cases: the tolerance is 0.25; atol = 0 cases: |y| from {1, 2, 4, 8}.)
At one `special` element - the planted index, else element 0 - term j holds j + 1, y0 = -0.5 (-1) and y1 = -3.5 (-4): a
dropped or swapped term, a missing fabs and |y0| for the maximum all change that element's ratio whatever the draw gives.

`real`.  N(0, 1) operands; coefficients like a tableau's (1 for y, then h = 0.37 times dopri5's weights, both signs, three
decades); rtol = 1e-3, atol = 1e-4.  Compared elementwise against float64 of the same float32 inputs, inside bounds derived
here (u = 2^-24, the unit roundoff of float32), never measured:
  combine       out = fma chain over nterms terms: nterms roundings, each at most u times a partial sum of |c_j t_ij|:
                |err_i| <= nterms u sum_j |c_j| |t_ij|   (the `reach` of tests/test_gpu_adaptive_methods.py); without the
                fused multiply-add the products round too, the first addition (to zero) does not: the same count.
  sum of N      float32 addends in any order (N - 1 additions, each rounding at most u times a partial sum of |x|; zeros
                added on the way are exact): (N - 1) u sum |x|, times |scale| (a power of two here: exact), plus 2 u |result|
                for the scale and the accumulate.
  error sum     r_i = e_i / tol_i: the combine's error over tol_i, two roundings in tol_i and one in the division; with
                |r_i| <= sum_j |c_j t_ij| / tol_i:  delta_i = (nterms + 2) u sum_j |c_j| |t_ij| / tol_i + 2 u |r_i|, and
                |sum - ref| <= sum_i (2 |r_i| delta_i + delta_i^2) + 2^-50 ref for the float64 additions.
  at            of gode_reduce_segments_f32: sum over the T time columns of (column sum) * w: each column sum as above, then a
                chain of fused multiply-adds per lane and five shuffle additions: (n_part - 1 + T + 5) u sum_c |w_c| sum_p |x_pc|.
"""
import functools
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24

# ---- the limits the routes branch on (graph_odenet_amd/csrc/rk.hip; line numbers of that file) ---------------------------
THREADS = 256             # :14 ... every kernel is __launch_bounds__(256) and launched with dim3(256)
LC_MAX_BLOCKS = 8192      # :509, :512, :536 `if (blocks > 8192) blocks = 8192;` - the combines' grid cap
RED_BLOCKS = 1024         # :12 `constexpr int RED_BLOCKS = 1024;`
RED_PER_BLOCK = 1024      # :455 red_blocks(n) = min(ceil(n / 1024), RED_BLOCKS), at least 1
PARTS4_MIN_LEN = 4096     # :666 reduce_parts4: len >= 4096 && n_part >= 64 && len % 4 == 0 && out, part 16-byte aligned
PARTS4_MIN_PARTS = 64
PARTS_GROUPS = 8          # :244-256 reduce_parts_kernel: 8 part-groups x 32 outputs, four loads in flight (`p + 24 < n_part`)
PARTS4_GROUPS = 16        # :349-369 reduce_parts4_kernel: 16 part-groups x 16 float4, four loads in flight (`p + 48 < n_part`)
PARTS_IN_FLIGHT = 4
COLSUM_ROWS = 256         # :492 colsum_blocks(n_rows) = min(ceil(n_rows / 256), 1024), at least 1; rpb = ceil(n_rows / blocks)
COLSUM_MAX_BLOCKS = 1024  # :494
WIDE_MIN_D = 512          # :749 the wide route: d >= 512 && n_rows <= 4 * d
WIDE_ROWS_PER_D = 4
COLSUM4_MAX_D = 1024      # :734, :756 colsum4: d % 4 == 0 && d <= 1024 && X, scratch 16-byte aligned
COLSUM_HALF = 256         # :429 colsum_kernel: `if (d <= 256)` threads share rows, else a thread owns columns c, c + 256, ...
WIDE_TRIP = 64            # :472 colsum_wide_kernel: `r + 56 < n_rows; r += 64` - eight loads in flight in each of 8 row groups
WIDE_GROUPS = 8
MAX_TERMS = 8             # include/graphode.h GODE_MAX_TERMS
MAX_SEGS = 8              # include/graphode.h GODE_MAX_REDUCE_SEGS
SEG_COLS = 32             # :295, :319 32 outputs (time block: 32 columns a trip) per block
E_NULLPTR, E_SHAPE, E_RANGE = -1, -2, -4
# 16-byte forms: lincomb (:507, :531) n % 4 == 0, out and every term aligned; error sums (:570, :630, :649) n % 4 == 0, y0, y1 (y)
# and every term aligned.


def red_blocks(n):
    return max(1, min(-(-n // RED_PER_BLOCK), RED_BLOCKS))


def colsum_blocks(n_rows):
    return max(1, min(-(-n_rows // COLSUM_ROWS), COLSUM_MAX_BLOCKS))


def colsum_rpb(n_rows):
    nb = colsum_blocks(n_rows)
    return max(-(-n_rows // nb), 1)


def lincomb_grid(n, vec):
    """(work items, blocks) of gode_lincomb_f32: a work item is a float4 in the 16-byte form, else a float."""
    work = n // 4 if vec else n
    return work, min(-(-work // THREADS), LC_MAX_BLOCKS)


def kept_parts(n_part, groups, drop_tail=False):
    """Partial rows a reduce_parts kernel with `groups` part-groups adds, group by group: four in flight, then a tail."""
    kept, unrolled, tail = [], False, False
    for q in range(groups):
        p = q
        while p + 3 * groups < n_part:
            kept += [p, p + groups, p + 2 * groups, p + 3 * groups]
            p += PARTS_IN_FLIGHT * groups
            unrolled = True
        while p < n_part:
            tail = True
            if not drop_tail:
                kept.append(p)
            p += groups
    return sorted(kept), unrolled, tail


class Case:
    def __init__(self, family, name, reaches, **kw):
        self.family, self.name, self.reaches = family, name, frozenset(reaches)
        self.__dict__.update(kw)

    def route(self):
        return frozenset(ROUTERS[self.family](self))

    @property
    def id(self):
        return "%s/%s" % (self.family, self.name)

    def __repr__(self):
        return self.id


# ---- routes, from the numbers above --------------------------------------------------------------------------------------
def lincomb_vec(c):
    return c.n % 4 == 0 and not c.mis


def lincomb_route(c):
    form = "lincomb4" if lincomb_vec(c) else "lincomb1"
    work, blocks = lincomb_grid(c.n, lincomb_vec(c))
    tags = {form, "%s:terms%d" % (form, c.nterms)}
    if work > blocks * THREADS:
        tags.add(form + ":wrap")
    if c.inplace is not None:
        tags.add("inplace:%s" % ("first" if c.inplace == 0 else "last"))
    return tags | {"misaligned:" + m for m in c.mis}


def err_vec(c):
    return c.n % 4 == 0 and not c.mis


def err_route(c):
    form = "ratio4" if err_vec(c) else "ratio1"
    work, nb = (c.n // 4 if err_vec(c) else c.n), red_blocks(c.n)
    tags = {"%s<%d>" % (form, c.mode), "%s:terms%d" % (form, c.nterms)}
    if work > nb * THREADS:
        tags.add(form + ":wrap")
    if nb == RED_BLOCKS:
        tags.add("blocks1024")
    if c.rtol == 0:
        tags.add("rtol0")
    if c.atol == 0:
        tags.add("atol0")
    if c.plant is not None:
        tags.add("planted")
    return tags | {"misaligned:" + m for m in c.mis}


def multi_route(c):
    vec = lincomb_vec if c.family == "lincomb_multi" else err_vec
    forms = {vec(k) for k in c.comps if k.n > 0}
    tags = {"count%d" % len(c.comps), "mixed_forms" if len(forms) == 2 else "one_form"}
    if any(k.n == 0 for k in c.comps[1:-1]):
        tags.add("empty_middle")
    if any(k.n == 1 for k in c.comps):
        tags.add("length1")
    if any(getattr(k, "inplace", None) is not None for k in c.comps):
        tags.add("inplace")
    if c.family == "err_multi" and max(red_blocks(k.n) for k in c.comps) == RED_BLOCKS * min(red_blocks(k.n) for k in c.comps):
        tags.add("nb_x1024")
    return tags


def parts_vec(c):
    return c.len >= PARTS4_MIN_LEN and c.n_part >= PARTS4_MIN_PARTS and c.len % 4 == 0 and not c.mis_out


def parts_route(c):
    vec = parts_vec(c) and c.family == "parts"                 # gode_reduce_parts2_f32 has the scalar kernel alone
    _, unrolled, tail = kept_parts(c.n_part, PARTS4_GROUPS if vec else PARTS_GROUPS)
    tags = {"parts4" if vec else "parts", "acc" if c.acc else "over", "scale%g" % c.scale}
    if unrolled:
        tags.add("in_flight4")
    if tail:
        tags.add("tail")
    if c.n_part == 0:
        tags.add("no_parts")
    if c.len % (64 if vec else 32):
        tags.add("partial_block")
    if c.mis_out:
        tags.add("misaligned:out")
    return tags


def segs_route(c):
    time = [s for s in c.segs if s["wrow"] and s["time_len"] > 0]
    tags = {"segs%d" % len(c.segs), "time%d" % len(time)}
    for s in c.segs:
        _, unrolled, tail = kept_parts(s["n_part"], PARTS_GROUPS)
        if unrolled:
            tags.add("in_flight4")
        if tail:
            tags.add("tail")
        if s["n_part"] == 0:
            tags.add("no_parts")
        if s["cs"] > 1:
            tags.add("col_stride%d" % s["cs"])
        if s["ld"] > s["col0"] + (s["len"] - 1) * s["cs"] + 1:
            tags.add("ld_surplus")
        if s["wrow"] and s["time_len"] == 0:
            tags.add("wrow_without_time")
        if s in time:
            tags.add("time_len==len" if s["time_len"] == s["len"] else "time_len<len")
            if s["time_len"] > SEG_COLS:
                tags.add("time_trips2")
    if c.at_null:
        tags.add("at_null")
    return tags


def colsum_wide(c):
    return c.d >= WIDE_MIN_D and c.n_rows <= WIDE_ROWS_PER_D * c.d


def colsum_block_kernel(c):
    if c.d % 4 == 0 and c.d <= COLSUM4_MAX_D and not c.mis_x:
        return "colsum4"
    return "colsum<=256" if c.d <= COLSUM_HALF else "colsum>256"


def colsum_route(c):
    """`f32:` what gode_colsum_f32 runs, `parts:` what gode_colsum_parts_f32 runs (it has no wide route)."""
    k = colsum_block_kernel(c)
    nb, rpb = colsum_blocks(c.n_rows), colsum_rpb(c.n_rows)
    tags = {"parts:" + k, "f32:wide" if colsum_wide(c) else "f32:" + k, "acc" if c.acc else "over", "scale%g" % c.scale}
    if colsum_wide(c):
        if c.n_rows > WIDE_TRIP - WIDE_GROUPS:
            tags.add("wide:trip64")
        if c.n_rows % WIDE_TRIP:
            tags.add("wide:tail")
        if c.d % 32:
            tags.add("wide:partial_block")
    if k == "colsum4":
        rows_par = THREADS // (c.d // 4)
        if THREADS % (c.d // 4):
            tags.add("colsum4:idle_threads")
        if rpb > 3 * rows_par:
            tags.add("colsum4:in_flight4")
        if rows_par == 1:
            tags.add("colsum4:one_row")
        if rows_par == THREADS:
            tags.add("colsum4:256_rows")
    if k == "colsum<=256" and THREADS % c.d:
        tags.add("colsum:idle_threads")
    if c.n_rows == 0:
        tags.add("no_rows")
    if c.n_rows > 0 and (nb - 1) * rpb >= c.n_rows:
        tags.add("blocks_past_end")
    if nb == COLSUM_MAX_BLOCKS:
        tags.add("blocks1024")
    if c.mis_x:
        tags.add("misaligned:X")
    return tags


ROUTERS = {"lincomb": lincomb_route, "err": err_route, "lincomb_multi": multi_route, "err_multi": multi_route, "parts": parts_route,
           "parts2": parts_route, "segs": segs_route, "colsum": colsum_route}

# every tag some case has to reach
ROUTE_TABLE = {
    "lincomb": ["lincomb4", "lincomb1", "lincomb4:wrap", "lincomb1:wrap", "inplace:first", "inplace:last", "misaligned:out",
                "misaligned:last", "misaligned:all"] + ["lincomb%d:terms%d" % (f, k) for f in (1, 4) for k in range(1, 9)],
    "lincomb_multi": ["count1", "count2", "count3", "count4", "mixed_forms", "one_form", "empty_middle", "length1", "inplace"],
    "err": ["ratio4<0>", "ratio4<1>", "ratio1<0>", "ratio1<1>", "ratio4:wrap", "ratio1:wrap", "blocks1024", "rtol0", "atol0", "planted",
            "misaligned:y0", "misaligned:y1", "misaligned:term"] + ["ratio%d:terms%d" % (f, k) for f in (1, 4) for k in range(1, 9)],
    "err_multi": ["count1", "count2", "count3", "count4", "mixed_forms", "one_form", "length1", "nb_x1024"],
    "parts": ["parts4", "parts", "acc", "over", "scale1", "scale-0.5", "scale0", "in_flight4", "tail", "no_parts", "partial_block",
              "misaligned:out"],
    "parts2": ["parts", "acc", "over", "scale1", "scale-0.5", "in_flight4", "tail", "partial_block"],
    "segs": ["segs1", "segs8", "time0", "time1", "time2", "in_flight4", "tail", "no_parts", "col_stride2", "col_stride3", "ld_surplus",
             "wrow_without_time", "time_len==len", "time_len<len", "time_trips2", "at_null"],
    "colsum": ["f32:colsum4", "f32:colsum<=256", "f32:colsum>256", "f32:wide", "parts:colsum4", "parts:colsum<=256", "parts:colsum>256",
               "wide:trip64", "wide:tail", "wide:partial_block", "colsum4:idle_threads", "colsum4:in_flight4", "colsum4:one_row",
               "colsum4:256_rows", "colsum:idle_threads", "no_rows", "blocks_past_end", "blocks1024", "misaligned:X", "acc", "over",
               "scale1", "scale-0.5", "scale0"],
}

# ---- cases ---------------------------------------------------------------------------------------------------------------
LC_N = ((1, 1), (3, 1), (4, 4), (5, 1), (255, 1), (256, 4), (257, 1), (1023, 1), (1024, 4), (1028, 4))      # (n, form)
LC_WRAP1_N = 2097153      # LC_MAX_BLOCKS * THREADS + 1: the scalar form's first wrap
LC_WRAP4_N = 8388612      # 4 * (LC_MAX_BLOCKS * THREADS + 1): the 16-byte form wraps with one trailing float4


def _lc(name, n, nterms, form, inplace=None, mis=(), wrap=False):
    f = "lincomb%d" % form
    tags = {f, "%s:terms%d" % (f, nterms)} | {"misaligned:" + m for m in mis}
    if wrap:
        tags.add(f + ":wrap")
    if inplace is not None:
        tags.add("inplace:%s" % ("first" if inplace == 0 else "last"))
    return Case("lincomb", name, tags, n=n, nterms=nterms, inplace=inplace, mis=frozenset(mis))


LINCOMB_CASES = [_lc("n%d" % n, n, 3, form) for n, form in LC_N]
LINCOMB_CASES += [_lc("wrap1", LC_WRAP1_N, 3, 1, wrap=True), _lc("wrap4", LC_WRAP4_N, 2, 4, wrap=True)]
LINCOMB_CASES += [_lc("terms%d_n1028" % k, 1028, k, 4) for k in range(1, 9)] + [_lc("terms%d_n1023" % k, 1023, k, 1) for k in range(1, 9)]
LINCOMB_CASES += [_lc("inplace0_n1028", 1028, 4, 4, inplace=0), _lc("inplacelast_n1028", 1028, 4, 4, inplace="last"),
                  _lc("inplace0_n257", 257, 8, 1, inplace=0), _lc("inplacelast_n257", 257, 8, 1, inplace="last"),
                  _lc("mis_out_n1028", 1028, 3, 1, mis=("out",)), _lc("mis_last_n1028", 1028, 3, 1, mis=("last",)),
                  _lc("mis_all_n1028", 1028, 8, 1, mis=("all",)), _lc("mis_all_n257", 257, 2, 1, mis=("all",))]


def _comp(name, n, nterms, inplace=None, mis=()):
    return Case("lincomb", "multi_" + name, (), n=n, nterms=nterms, inplace=inplace, mis=frozenset(mis))


LINCOMB_MULTI_CASES = [
    Case("lincomb_multi", "count1", {"count1", "one_form"}, comps=[_comp("c1a", 1028, 3)]),
    Case("lincomb_multi", "count2", {"count2", "mixed_forms"}, comps=[_comp("c2a", 1024, 8), _comp("c2b", 5, 2)]),
    Case("lincomb_multi", "count3", {"count3", "mixed_forms", "length1", "inplace"},
         comps=[_comp("c3a", 1023, 4), _comp("c3b", 1, 1), _comp("c3c", 256, 3, inplace=0)]),
    Case("lincomb_multi", "count4", {"count4", "mixed_forms", "empty_middle"},
         comps=[_comp("c4a", 1028, 2), _comp("c4b", 0, 1), _comp("c4c", 257, 5), _comp("c4d", 4, 7)]),
    Case("lincomb_multi", "count4_scalar", {"count4", "one_form", "length1"},
         comps=[_comp("c5a", 1, 2), _comp("c5b", 1028, 3, mis=("out",)), _comp("c5c", 3, 8), _comp("c5d", 513, 1)]),
]

ERR_N = ((1, 1), (3, 1), (4, 4), (1023, 1), (1024, 4), (1025, 1), (1028, 4), (4096, 4))
ERR_FULL_N = 1048576      # RED_BLOCKS * THREADS float4: 1024 blocks, the 16-byte form does not wrap
ERR_WRAP4_N = 1048580     # one float4 more: it wraps
ERR_WRAP1_N = 1048577     # the scalar form at 1024 blocks (stride 262144: it has wrapped four times)


def _err(name, mode, n, nterms, form, mis=(), rtol=None, atol=None, plant=None, wrap=None):
    f = "ratio%d" % form
    tags = {"%s<%d>" % (f, mode), "%s:terms%d" % (f, nterms)} | {"misaligned:" + m for m in mis}
    if wrap if wrap is not None else (form == 1 and n > red_blocks(n) * THREADS):
        tags.add(f + ":wrap")
    if n >= (RED_BLOCKS - 1) * RED_PER_BLOCK + 1:
        tags.add("blocks1024")
    for v, t in ((rtol, "rtol0"), (atol, "atol0")):
        if v == 0:
            tags.add(t)
    if plant is not None:
        tags.add("planted")
    return Case("err", "%s_m%d" % (name, mode), tags, mode=mode, n=n, nterms=nterms, mis=frozenset(mis), rtol=rtol, atol=atol, plant=plant)


# planted: (n, form, index, what the index is)
PLANTS = ((1025, 1, 0, "first"), (1025, 1, 1024, "last = first after the last whole float4"), (1025, 1, 1023, "last of the last whole float4"),
          (1025, 1, 255, "end of block 0"), (1025, 1, 256, "start of block 1"), (1025, 1, 511, "before the wrap"), (1025, 1, 512, "after the wrap"),
          (1028, 4, 0, "first"), (1028, 4, 1027, "last = last of the last whole float4"), (1028, 4, 1023, "end of block 0"),
          (1028, 4, 1024, "start of block 1"),
          (ERR_WRAP4_N, 4, 1048575, "before the wrap"), (ERR_WRAP4_N, 4, 1048576, "after the wrap"), (ERR_WRAP4_N, 4, 1048579, "last"),
          (ERR_WRAP1_N, 1, 262143, "before the first wrap"), (ERR_WRAP1_N, 1, 262144, "after the first wrap"),
          (ERR_WRAP1_N, 1, 1048575, "last of the last whole float4"), (ERR_WRAP1_N, 1, 1048576, "last = first after the last whole float4"))

ERR_CASES = []
for _m in (0, 1):
    ERR_CASES += [_err("n%d" % n, _m, n, 3, form) for n, form in ERR_N]
    ERR_CASES += [_err("full", _m, ERR_FULL_N, 2, 4, wrap=False), _err("wrap4", _m, ERR_WRAP4_N, 2, 4, wrap=True),
                  _err("wrap1", _m, ERR_WRAP1_N, 2, 1)]
    ERR_CASES += [_err("terms%d_n1028" % k, _m, 1028, k, 4) for k in range(1, 9)] + [_err("terms%d_n1025" % k, _m, 1025, k, 1) for k in range(1, 9)]
    ERR_CASES += [_err("mis_y0_n1028", _m, 1028, 3, 1, mis=("y0",)), _err("mis_term_n1028", _m, 1028, 3, 1, mis=("term",)),
                  _err("rtol0_n1028", _m, 1028, 3, 4, rtol=0.0), _err("rtol0_n1025", _m, 1025, 3, 1, rtol=0.0),
                  _err("atol0_n1028", _m, 1028, 3, 4, atol=0.0), _err("atol0_n1025", _m, 1025, 3, 1, atol=0.0)]
    ERR_CASES += [_err("plant%d_n%d" % (i, n), _m, n, 2, form, plant=i, wrap=(n == ERR_WRAP4_N) if form == 4 else None)
                  for n, form, i, _ in PLANTS]
ERR_CASES += [_err("mis_y1_n1028", 0, 1028, 3, 1, mis=("y1",))]                  # gode_rk_scaled_sumsq_f32 has no y1


def _ecomp(name, n, nterms, mis=()):
    return Case("err", "multi_" + name, (), mode=0, n=n, nterms=nterms, mis=frozenset(mis), rtol=None, atol=None, plant=None)


ERR_MULTI_CASES = [
    Case("err_multi", "count1", {"count1", "one_form"}, comps=[_ecomp("c1a", 1028, 3)]),
    Case("err_multi", "count2", {"count2", "mixed_forms"}, comps=[_ecomp("c2a", 1024, 8), _ecomp("c2b", 1025, 2)]),
    Case("err_multi", "count3", {"count3", "mixed_forms", "length1", "nb_x1024"},
         comps=[_ecomp("c3a", 1, 2), _ecomp("c3b", ERR_WRAP4_N, 2), _ecomp("c3c", 3, 4)]),
    Case("err_multi", "count3_mixed", {"count3", "mixed_forms", "length1", "nb_x1024"},
         comps=[_ecomp("c5a", ERR_WRAP4_N, 2), _ecomp("c5b", 4096, 2), _ecomp("c5c", 1, 2)]),
    Case("err_multi", "count4", {"count4", "mixed_forms"},
         comps=[_ecomp("c4a", 1023, 5), _ecomp("c4b", 1028, 3, mis=("y1",)), _ecomp("c4c", 4, 7), _ecomp("c4d", 3, 1)]),
]


def _parts(n_part, length, acc, scale, tags, mis_out=False, family="parts"):
    name = "%dx%d_acc%d_scale%g%s" % (n_part, length, acc, scale, "_mis_out" if mis_out else "")
    tags = set(tags.split()) | {"acc" if acc else "over", "scale%g" % scale} | ({"misaligned:out"} if mis_out else set())
    return Case(family, name, tags, n_part=n_part, len=length, acc=acc, scale=scale, mis_out=mis_out)


PARTS_CASES = [
    _parts(0, 33, 0, 1.0, "parts no_parts partial_block"), _parts(0, 32, 1, -0.5, "parts no_parts"),
    _parts(1, 33, 1, 1.0, "parts tail partial_block"), _parts(7, 31, 0, -0.5, "parts tail partial_block"),
    _parts(8, 32, 1, 0.0, "parts tail"), _parts(9, 1, 0, 0.0, "parts tail partial_block"), _parts(9, 33, 1, -0.5, "parts tail partial_block"),
    _parts(24, 33, 0, 1.0, "parts tail partial_block"), _parts(25, 33, 1, -0.5, "parts in_flight4 tail partial_block"),
    _parts(32, 32, 0, -0.5, "parts in_flight4"), _parts(33, 31, 1, 1.0, "parts in_flight4 tail partial_block"),
    _parts(37, 1000, 0, 1.0, "parts in_flight4 tail partial_block"), _parts(57, 1000, 1, -0.5, "parts in_flight4 tail partial_block"),
    _parts(63, 4096, 0, 1.0, "parts in_flight4 tail"), _parts(64, 4097, 1, -0.5, "parts in_flight4 partial_block"),
    _parts(64, 4092, 0, -0.5, "parts in_flight4 partial_block"), _parts(64, 4096, 1, 1.0, "parts in_flight4", mis_out=True),
    _parts(128, 1000, 1, 1.0, "parts in_flight4 partial_block"), _parts(512, 33, 0, 1.0, "parts in_flight4 partial_block"),
    _parts(64, 4096, 0, 1.0, "parts4 in_flight4"), _parts(64, 4096, 1, -0.5, "parts4 in_flight4"),
    _parts(64, 4100, 1, 1.0, "parts4 in_flight4 partial_block"), _parts(65, 4096, 0, -0.5, "parts4 in_flight4 tail"),
    _parts(79, 4096, 1, 0.0, "parts4 in_flight4 tail"), _parts(80, 4100, 0, 1.0, "parts4 in_flight4 tail partial_block"),
    _parts(81, 4096, 1, -0.5, "parts4 in_flight4 tail"), _parts(112, 4096, 0, 0.0, "parts4 in_flight4 tail"),
    _parts(113, 4100, 1, 1.0, "parts4 in_flight4 tail partial_block"), _parts(128, 4096, 0, -0.5, "parts4 in_flight4"),
    _parts(512, 4096, 1, 1.0, "parts4 in_flight4"),
]
PARTS2_CASES = [_parts(37, 33, 0, 1.0, "parts in_flight4 tail partial_block", family="parts2"),
                _parts(9, 1, 1, -0.5, "parts tail partial_block", family="parts2")]


def _seg(n_part, length, col0=0, cs=1, ld=None, wrow=False, time_len=0):
    need = col0 + (length - 1) * cs + 1
    return dict(n_part=n_part, len=length, col0=col0, cs=cs, ld=need if ld is None else ld, wrow=wrow, time_len=time_len)


SEG_SURPLUS = 3           # every output is this much longer than its segment: the surplus stays NaN
SEGS_CASES = [
    Case("segs", "one", {"segs1", "time0", "tail", "at_null"}, segs=[_seg(1, 1)], at_null=True),
    Case("segs", "eight", {"segs8", "time0", "tail", "in_flight4", "no_parts", "col_stride2", "col_stride3", "ld_surplus", "at_null"},
         segs=[_seg(0, 1), _seg(1, 31), _seg(8, 32, col0=2, cs=2), _seg(9, 33, col0=1, cs=3, ld=110), _seg(33, 300), _seg(33, 33, ld=40),
               _seg(9, 32, col0=5), _seg(1, 31, cs=2)], at_null=True),
    Case("segs", "time_one", {"segs1", "time1", "tail", "time_len==len"}, segs=[_seg(9, 32, wrow=True, time_len=32)], at_null=False),
    Case("segs", "time_two", {"segs8", "time2", "tail", "in_flight4", "no_parts", "col_stride2", "col_stride3", "ld_surplus",
                              "wrow_without_time", "time_len<len", "time_len==len", "time_trips2"},
         segs=[_seg(33, 300, wrow=True, time_len=33), _seg(8, 31, wrow=True, time_len=0), _seg(9, 33),
               _seg(0, 32), _seg(1, 1, col0=2, cs=3, ld=4), _seg(33, 33, col0=3, cs=2, ld=80, wrow=True, time_len=33), _seg(8, 31), _seg(9, 300, col0=1)],
         at_null=False),
    Case("segs", "wrow_without_time", {"segs1", "time0", "tail", "wrow_without_time", "at_null"},
         segs=[_seg(9, 33, wrow=True, time_len=0)], at_null=True),
]


def _cs(n_rows, d, acc, scale, tags, mis_x=False):
    name = "%dx%d_acc%d_scale%g%s" % (n_rows, d, acc, scale, "_mis_x" if mis_x else "")
    tags = set(tags.split()) | {"acc" if acc else "over", "scale%g" % scale} | ({"misaligned:X"} if mis_x else set())
    return Case("colsum", name, tags, n_rows=n_rows, d=d, acc=acc, scale=scale, mis_x=mis_x)


_C4, _CL, _CG = "f32:colsum4 parts:colsum4 ", "f32:colsum<=256 parts:colsum<=256 ", "f32:colsum>256 parts:colsum>256 "
_AS = ((0, 1.0), (1, -0.5), (1, 1.0), (0, -0.5), (1, 0.0), (0, 0.0))
COLSUM_BIG_ROWS = 262400  # 1024 blocks of rpb = 257 rows: blocks 1022 and 1023 start past the end
COLSUM_CASES = [
    # colsum4_kernel
    _cs(257, 4, 0, 1.0, _C4 + "colsum4:256_rows"), _cs(513, 12, 1, -0.5, _C4 + "colsum4:idle_threads"),
    _cs(256, 128, 1, 1.0, _C4 + "colsum4:in_flight4"), _cs(0, 128, 0, -0.5, _C4 + "no_rows"), _cs(1, 128, 1, 0.0, _C4),
    _cs(255, 300, 0, 0.0, _C4 + "colsum4:idle_threads colsum4:in_flight4"), _cs(2, 300, 1, -0.5, _C4 + "colsum4:idle_threads"),
    _cs(4097, 1024, 0, 1.0, _C4 + "colsum4:one_row colsum4:in_flight4"), _cs(2049, 512, 1, 1.0, _C4 + "colsum4:in_flight4"),
    _cs(COLSUM_BIG_ROWS, 4, 1, -0.5, _C4 + "colsum4:256_rows blocks_past_end blocks1024"),
    # colsum_kernel, d <= 256
    _cs(513, 1, 0, 1.0, _CL), _cs(257, 3, 1, -0.5, _CL + "colsum:idle_threads"), _cs(0, 3, 1, 1.0, _CL + "colsum:idle_threads no_rows"),
    _cs(256, 7, 0, -0.5, _CL + "colsum:idle_threads"), _cs(1, 7, 0, 1.0, _CL + "colsum:idle_threads"),
    _cs(255, 73, 1, 0.0, _CL + "colsum:idle_threads"), _cs(2, 255, 0, 0.0, _CL + "colsum:idle_threads"),
    _cs(513, 256, 1, -0.5, _CL, mis_x=True), _cs(257, 12, 0, 1.0, _CL + "colsum:idle_threads", mis_x=True),
    # colsum_kernel, d > 256
    _cs(513, 257, 0, 1.0, _CG), _cs(257, 301, 1, -0.5, _CG), _cs(255, 511, 1, 1.0, _CG), _cs(2053, 513, 0, -0.5, _CG),
    _cs(4113, 1028, 1, 1.0, _CG),
    # colsum_wide_kernel (gode_colsum_parts_f32 has no such route: it runs the row-block kernel of the same d)
    _cs(2048, 512, 0, -0.5, "f32:wide parts:colsum4 wide:trip64 colsum4:in_flight4"),
]
for _k, _n in enumerate((0, 1, 7, 8, 9, 63, 64, 65, 127, 128)):
    for _d in (513, 2667):
        _t = "f32:wide parts:colsum>256 wide:partial_block" + (" wide:trip64" if _n >= 57 else "") + (" wide:tail" if _n % 64 else "") + \
             (" no_rows" if _n == 0 else "")
        COLSUM_CASES.append(_cs(_n, _d, *_AS[(_k + (_d > 513)) % 6], _t))

FAMILIES = {"lincomb": LINCOMB_CASES, "lincomb_multi": LINCOMB_MULTI_CASES, "err": ERR_CASES, "err_multi": ERR_MULTI_CASES,
            "parts": PARTS_CASES, "parts2": PARTS2_CASES, "segs": SEGS_CASES, "colsum": COLSUM_CASES}
ALL_CASES = [c for cases in FAMILIES.values() for c in cases]
BY_ID = {c.id: c for c in ALL_CASES}
LARGE_N = 1 << 20         # cases from here on are the grid-stride wraps (and the 1024-block column sum)

# ---- data ----------------------------------------------------------------------------------------------------------------
EXACT_COEF = (1.0, -0.5, 2.0, 0.0, 0.25, -4.0, 0.5, -2.0)
H = 0.37
REAL_COEF = (1.0, H * 35 / 384, -H * 2187 / 6784, H * 500 / 1113, H * 125 / 192, -H * 0.0123, H * 11 / 84, -H * 1.7)
EXACT_ERR_COEF = (4.0, -8.0, 8.0, 4.0, -4.0, 8.0, 4.0, -8.0)
REAL_ERR_COEF = (H * 71 / 57600, -H * 71 / 16695, H * 71 / 1920, -H * 17253 / 339200, H * 22 / 525, -H / 40, H * 0.5, -H * 0.01)
EXACT_TOL, REAL_TOL = (0.5, 0.25), (1e-3, 1e-4)            # (rtol, atol)
EXACT_T, REAL_T = 0.5, 0.37                                # the time of gode_reduce_segments_f32


def _rng(case, kind):
    return np.random.RandomState(zlib.crc32(("%s/%s" % (case.id, kind)).encode()))


def _signed(rng, shape):
    return (rng.randint(1, 9, shape) * rng.choice((-1, 1), shape)).astype(F32)


def _columns(rng, rows, cols, kind):
    """rows x cols: exact - magnitudes 1 .. 8 with one sign per column; real - N(0, 1)."""
    if kind == "real":
        return rng.standard_normal((rows, cols)).astype(F32)
    return (rng.randint(1, 9, (rows, cols)) * rng.choice((-1, 1), (1, cols))).astype(F32)


def _vector(rng, n, kind):
    return rng.standard_normal(n).astype(F32) if kind == "real" else _signed(rng, n)


def _design_wrap(case, terms, vec, blocks):
    """exact data: the last elements of the two work items on either side of the first grid-stride wrap hold term j = j + 1,
    but for term 0 after the wrap (2): whatever the draw, the two combinations differ by coefficient 0 and, under equal y, so
    do the squared ratios (EXACT_ERR_COEF: 4, -12, 12, 28, 8, 56, 84, 20 before, 4 more after).  Returns the two indices."""
    unit = 4 if vec else 1
    first = blocks * THREADS * unit                              # first element of the second trip
    if case.n // unit * unit <= first:
        return ()
    pair = (first - 1, first + unit - 1)
    for i in pair:
        for j, t in enumerate(terms):
            t[i] = j + 1
    terms[0][pair[1]] = 2
    return pair


@functools.lru_cache(maxsize=16)
def inputs(case, kind):
    rng = _rng(case, kind)
    fam = case.family
    if fam in ("lincomb_multi", "err_multi"):
        return {"comps": [inputs(k, kind) for k in case.comps]}
    if fam == "lincomb":
        terms = [_vector(rng, case.n, kind) for _ in range(case.nterms)]
        if kind == "exact" and case.n:
            for j, t in enumerate(terms):
                t[0] = j + 1
            _design_wrap(case, terms, lincomb_vec(case), lincomb_grid(case.n, lincomb_vec(case))[1])
        return {"coef": np.array((EXACT_COEF if kind == "exact" else REAL_COEF)[:case.nterms], F32), "terms": terms}
    if fam == "err":
        n, s = case.n, (case.plant if case.plant is not None else 0)
        rtol, atol = EXACT_TOL if kind == "exact" else REAL_TOL
        rtol, atol = (rtol if case.rtol is None else case.rtol), (atol if case.atol is None else case.atol)
        terms = [_vector(rng, n, kind) for _ in range(case.nterms)]
        if kind == "exact":
            mags = np.array((1.0, 2.0, 4.0, 8.0) if atol == 0 else (0.5, 1.5, 3.5, 7.5), F32)
            i0 = rng.randint(0, 4, n)
            i1 = (i0 + rng.randint(1, 4, n)) % 4                               # never the same magnitude
            y0, y1 = mags[i0] * rng.choice((-1, 1), n).astype(F32), mags[i1] * rng.choice((-1, 1), n).astype(F32)
            y0[s], y1[s] = -mags[0], -mags[2]
            for j, t in enumerate(terms):
                t[s] = j + 1
            if case.plant is None:
                for i in _design_wrap(case, terms, err_vec(case), red_blocks(n)):
                    y0[i], y1[i] = -mags[0], -mags[2]
        else:
            y0, y1 = _vector(rng, n, kind), _vector(rng, n, kind)
        if case.plant is not None:
            for t in terms:
                keep = t[s]
                t[:] = 0
                t[s] = keep
        return {"coef": np.array((EXACT_ERR_COEF if kind == "exact" else REAL_ERR_COEF)[:case.nterms], F32), "terms": terms,
                "y0": y0.astype(F32), "y1": y1.astype(F32), "rtol": float(F32(rtol)), "atol": float(F32(atol))}
    if fam in ("parts", "parts2"):
        d = {"part": _columns(rng, case.n_part, case.len, kind), "out0": _vector(rng, case.len, kind)}
        if fam == "parts2":
            d.update(part_b=_columns(rng, case.n_part, case.len, kind), out0_b=_vector(rng, case.len, kind))
        return d
    if fam == "segs":
        segs = []
        for s in case.segs:
            w = _vector(rng, s["len"], kind)
            if kind == "exact":
                w = np.sign(w) * (1 + np.abs(w) % 4)
            segs.append({"part": _columns(rng, s["n_part"], s["ld"], kind), "w": w.astype(F32)})
        return {"segs": segs, "t": EXACT_T if kind == "exact" else REAL_T}
    if fam == "colsum":
        return {"X": _columns(rng, case.n_rows, case.d, kind), "out0": _vector(rng, case.d, kind)}
    raise KeyError(fam)


# ---- float64 reference and derived bounds: {quantity: (ref, bound)} ---------------------------------------------------------
def sum_ref(x, scale, acc, out0):
    """scale * column sums of x (+ out0): (ref, bound) by the 'sum of N' derivation of the module docstring."""
    x64 = x.astype(F64)
    ref = scale * x64.sum(0) + (out0.astype(F64) if acc else 0.0)
    bound = abs(scale) * max(x.shape[0] - 1, 0) * U * np.abs(x64).sum(0) + 2 * U * np.abs(ref)
    return ref, bound


def err_terms(case, d):
    """(r, delta) per element in float64: the ratio and its float32 error by the 'error sum' derivation."""
    e = sum(F64(c) * t.astype(F64) for c, t in zip(d["coef"], d["terms"]))
    reach = sum(abs(F64(c)) * np.abs(t.astype(F64)) for c, t in zip(d["coef"], d["terms"]))
    m = np.abs(d["y0"].astype(F64))
    if case.mode == 0:
        m = np.maximum(m, np.abs(d["y1"].astype(F64)))
    tol = d["atol"] + d["rtol"] * m
    r = e / tol
    return r, (case.nterms + 2) * U * reach / tol + 2 * U * np.abs(r)


def block_rows(n_rows):
    nb, rpb = colsum_blocks(n_rows), colsum_rpb(n_rows)
    return [(min(b * rpb, n_rows), min((b + 1) * rpb, n_rows)) for b in range(nb)]


@functools.lru_cache(maxsize=16)
def reference(case, kind):
    d, fam = inputs(case, kind), case.family
    if fam in ("lincomb_multi", "err_multi"):
        return {"comps": [reference(k, kind) for k in case.comps]}
    if fam == "lincomb":
        ref = sum((F64(c) * t.astype(F64) for c, t in zip(d["coef"], d["terms"])), np.zeros(case.n))
        reach = sum((abs(F64(c)) * np.abs(t.astype(F64)) for c, t in zip(d["coef"], d["terms"])), np.zeros(case.n))
        return {"out": (ref, case.nterms * U * reach)}
    if fam == "err":
        r, delta = err_terms(case, d)
        ref = float(np.sum(r * r))
        return {"sum": (ref, float(np.sum(2 * np.abs(r) * delta + delta * delta)) + 2.0 ** -50 * ref)}
    if fam == "parts":
        return {"out": sum_ref(d["part"], case.scale, case.acc, d["out0"])}
    if fam == "parts2":
        return {"out_a": sum_ref(d["part"], case.scale, case.acc, d["out0"]), "out_b": sum_ref(d["part_b"], case.scale, case.acc, d["out0_b"])}
    if fam == "colsum":
        res = {"out": sum_ref(d["X"], case.scale, case.acc, d["out0"])}
        blocks = [sum_ref(d["X"][a:b], 1.0, 0, None) for a, b in block_rows(case.n_rows)]
        res["parts"] = (np.stack([r for r, _ in blocks]), np.stack([b for _, b in blocks]))
        return res
    if fam == "segs":
        res, at, at_reach, n_time, np_max = {}, 0.0, 0.0, 0, 0
        for k, (s, sd) in enumerate(zip(case.segs, d["segs"])):
            cols = s["col0"] + np.arange(s["len"]) * s["cs"]
            ref, bound = sum_ref(sd["part"][:, cols], 1.0, 0, None)
            if s["wrow"] and s["time_len"] > 0:
                tl, w = s["time_len"], sd["w"].astype(F64)
                at += float(np.sum(ref[:tl] * w[:tl]))
                at_reach += float(np.sum(np.abs(sd["part"][:, cols[:tl]].astype(F64)).sum(0) * np.abs(w[:tl])))
                n_time, np_max = n_time + tl, max(np_max, s["n_part"])
                ref, bound = ref.copy(), bound.copy()
                ref[:tl] *= F64(F32(d["t"]))
                bound[:tl] = abs(d["t"]) * bound[:tl] + 2 * U * np.abs(ref[:tl])
            res["out%d" % k] = (ref, bound)
        if n_time:
            res["at"] = (at, (max(np_max - 1, 0) + n_time + 5) * U * at_reach)
        return res
    raise KeyError(fam)


# ---- the comparisons the GPU test uses --------------------------------------------------------------------------------------
def exact_equal(got, ref):
    """got (float32 array or a float64 sum) is the float64 reference: rounded to float32 for arrays, == for sums."""
    if np.ndim(ref) == 0:
        return float(got) == float(ref)
    got = np.asarray(got)
    return got.shape == np.shape(ref) and not np.isnan(got).any() and np.array_equal(got, np.asarray(ref).astype(got.dtype))


def within(got, ref, bound):
    got64 = np.asarray(got, F64)
    if got64.shape != np.shape(ref) or np.isnan(got64).any():
        return False
    return bool(np.all(np.abs(got64 - ref) <= bound))


def error_figures(got, ref, bound):
    """(the suite's metric max |got - ref| / max(1, max |ref|), the largest fraction of the derived bound used)."""
    diff = np.abs(np.asarray(got, F64) - ref)
    if diff.size == 0:
        return 0.0, 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(diff == 0, 0.0, diff / np.broadcast_to(np.asarray(bound, F64), diff.shape))
    return float(diff.max() / max(1.0, float(np.abs(ref).max()))), float(np.max(frac))


def exact_room(case):
    """exact data: (largest partial sum on absolute values) / granularity; below 2^24 (2^53 for the error sums) every order is exact."""
    d, fam = inputs(case, "exact"), case.family
    if fam == "lincomb":
        gran = min([abs(float(c)) for c in d["coef"] if c != 0] + [1.0])
        return float(sum((abs(float(c)) * np.abs(t) for c, t in zip(d["coef"], d["terms"])), np.zeros(case.n)).max(initial=0)) / gran
    if fam == "err":
        r, _ = err_terms(case, d)
        reach = sum(abs(F64(c)) * np.abs(t.astype(F64)) for c, t in zip(d["coef"], d["terms"]))
        assert reach.max() < 2 ** 10 and np.all(r == np.rint(r)) and np.all(reach % 4 == 0)
        m = np.abs(d["y0"]) if case.mode else np.maximum(np.abs(d["y0"]), np.abs(d["y1"]))
        assert set(np.unique(d["atol"] + d["rtol"] * m.astype(F64))) <= {0.25, 0.5, 1.0, 2.0, 4.0}
        tol = d["atol"] + d["rtol"] * m.astype(F64)
        return float(np.sum((reach / tol) ** 2))
    if fam in ("parts", "parts2", "colsum"):
        x = d["part"] if fam != "colsum" else d["X"]
        gran = min(abs(case.scale), 1.0) if case.scale else 1.0
        room = np.abs(x).sum(0).max(initial=0) * max(abs(case.scale), 1.0) + np.abs(d["out0"]).max()
        if fam == "parts2":
            room = max(room, np.abs(d["part_b"]).sum(0).max(initial=0) * max(abs(case.scale), 1.0) + np.abs(d["out0_b"]).max())
        return float(room) / gran
    if fam == "segs":
        room = 0.0
        for s, sd in zip(case.segs, d["segs"]):
            room += float((np.abs(sd["part"]).sum(0).max(initial=0)) * np.abs(sd["w"]).max() * max(s["time_len"], 1))
        return room / min(abs(d["t"]), 1.0)
    raise KeyError(fam)


# ---- float32 restatements of the kernels, right (mut = None) and wrong ------------------------------------------------------
MUTATIONS = ("drop_tail4", "drop_last_block", "dup_at_wrap", "drop_term8", "swap_coefs", "max_as_y0", "no_fabs", "swap_tols",
             "ignore_acc", "scale_acc", "drop_group_tail", "ignore_col_stride", "time_scale_past", "at_from_scaled", "short_last_block")
# the case whose REAL comparison rejects each mutation (test_rk_routes.py asserts it; the exact comparison rejects it on
# every case it touches)
MUTATION_REAL_CASE = {
    "drop_tail4": "err/n1025_m0", "drop_last_block": "err/n1028_m1", "dup_at_wrap": "err/plant1048576_n1048580_m0",
    "drop_term8": "lincomb/terms8_n1028", "swap_coefs": "lincomb/n1024", "max_as_y0": "err/n1024_m0", "no_fabs": "err/n1028_m1",
    "swap_tols": "err/n1023_m0", "ignore_acc": "parts/25x33_acc1_scale-0.5", "scale_acc": "colsum/513x12_acc1_scale-0.5",
    "drop_group_tail": "parts/65x4096_acc0_scale-0.5", "ignore_col_stride": "segs/eight", "time_scale_past": "segs/time_two",
    "at_from_scaled": "segs/time_one", "short_last_block": "colsum/257x4_acc0_scale1",
}


def touches(mut, case):
    """Whether the wrong kernel `mut` computes something else than the right one on this case's route."""
    fam = case.family
    if fam in ("lincomb", "err"):
        vec = lincomb_vec(case) if fam == "lincomb" else err_vec(case)
        work = case.n // 4 if vec else case.n
        blocks = lincomb_grid(case.n, vec)[1] if fam == "lincomb" else red_blocks(case.n)
        plant = getattr(case, "plant", None)
        live = plant is None                                    # a planted case has one live element
        at = None if live else (plant // 4 if vec else plant)
        if mut == "drop_tail4":
            return case.n % 4 != 0 and (live or plant >= case.n - case.n % 4)
        if mut == "drop_last_block":
            return case.n > 0 and (live or (at // THREADS) % blocks == blocks - 1)
        if mut == "dup_at_wrap":
            return work > blocks * THREADS and (live or at in (blocks * THREADS - 1, blocks * THREADS))
        if mut == "drop_term8":
            return case.nterms == 8
        if mut == "swap_coefs":
            return case.nterms >= 2
        if fam == "err" and mut == "max_as_y0":
            return case.mode == 0 and case.rtol != 0
        if fam == "err" and mut == "no_fabs":                   # atol = 0 under |y0| alone: only the ratio's sign changes
            return case.rtol != 0 and not (case.mode == 1 and case.atol == 0)
        return fam == "err" and mut == "swap_tols"
    if fam in ("parts", "parts2"):
        if mut == "ignore_acc":
            return bool(case.acc)
        if mut == "scale_acc":
            return bool(case.acc) and case.scale != 1
        return mut == "drop_group_tail" and case.scale != 0 and kept_parts(case.n_part, PARTS4_GROUPS if "parts4" in case.reaches else PARTS_GROUPS)[2]
    if fam == "colsum":
        if mut == "ignore_acc":
            return bool(case.acc)
        if mut == "scale_acc":
            return bool(case.acc) and case.scale != 1
        return mut == "short_last_block" and case.n_rows > 0       # the partials always; out too unless wide or scale == 0
    if fam == "segs":
        time = [s for s in case.segs if s["wrow"] and s["time_len"] > 0]
        if mut == "drop_group_tail":
            return any(kept_parts(s["n_part"], PARTS_GROUPS)[2] for s in case.segs)
        if mut == "ignore_col_stride":
            return any(s["cs"] > 1 and s["len"] > 1 and s["n_part"] > 0 for s in case.segs)
        if mut == "time_scale_past":
            return any(s["time_len"] < s["len"] and s["n_part"] > 0 for s in time)
        return mut == "at_from_scaled" and any(s["n_part"] > 0 for s in time)
    return False


def _lc32(coef, terms, n, mut):
    coef = [F32(c) for c in coef]
    if mut == "swap_coefs" and len(coef) >= 2:
        coef[0], coef[1] = coef[1], coef[0]
    k = len(terms) - 1 if (mut == "drop_term8" and len(terms) == MAX_TERMS) else len(terms)
    r = np.zeros(n, F32)
    for j in range(k):
        r = r + coef[j] * terms[j]                              # float32 product, float32 sum: no fused multiply-add
    return r


def _grid_view(n, vec, blocks, mut):
    """(kept: elements the grid visits, src: the element each visit reads) under a mutation of the grid-stride loop."""
    idx = np.arange(n)
    unit = 4 if vec else 1
    item = idx // unit
    kept, src = np.ones(n, bool), idx
    if mut == "drop_tail4":
        kept = idx < n - n % 4
    if mut == "drop_last_block":
        kept = (item // THREADS) % blocks != blocks - 1
    if mut == "dup_at_wrap" and (n // unit) > blocks * THREADS:
        src = np.where(item == blocks * THREADS, idx - unit, idx)     # the first item of the second trip reads the one before it
    return kept, src


def _sum32(x, order):
    """float32 column sums of x (rows x cols): sequential over the rows, or pairwise."""
    if x.shape[0] == 0:
        return np.zeros(x.shape[1], F32)
    if order == "seq":
        return np.cumsum(x, axis=0, dtype=F32)[-1]
    return np.sum(np.ascontiguousarray(x.T), axis=1, dtype=F32)


def _close32(s, scale, acc, out0, mut):
    if acc and mut == "scale_acc":
        return (out0 + s) * F32(scale)
    t = s * F32(scale)
    return out0 + t if (acc and mut != "ignore_acc") else t


def restate(case, kind, order="seq", mut=None):
    """What the kernels of this case compute, in float32 numpy without fused multiply-adds, sums in `order` ("seq" | "pair");
    mut: one of MUTATIONS (a wrong kernel).  Same keys as reference(); combines leave NaN where nothing is stored."""
    d, fam = inputs(case, kind), case.family
    if fam == "lincomb":
        vec = lincomb_vec(case)
        kept, src = _grid_view(case.n, vec, lincomb_grid(case.n, vec)[1], mut)
        return {"out": np.where(kept, _lc32(d["coef"], d["terms"], case.n, mut)[src], F32(np.nan)).astype(F32)}
    if fam == "err":
        kept, src = _grid_view(case.n, err_vec(case), red_blocks(case.n), mut)
        e = _lc32(d["coef"], d["terms"], case.n, mut)
        y0, y1 = (d["y0"], d["y1"]) if mut == "no_fabs" else (np.abs(d["y0"]), np.abs(d["y1"]))
        m = np.maximum(y0, y1) if (case.mode == 0 and mut != "max_as_y0") else y0
        rtol, atol = (F32(d["atol"]), F32(d["rtol"])) if mut == "swap_tols" else (F32(d["rtol"]), F32(d["atol"]))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = (e / (atol + rtol * m))[src][kept].astype(F64)
        sq = r * r
        return {"sum": float(np.cumsum(sq)[-1] if (order == "seq" and sq.size) else np.sum(sq))}
    if fam in ("parts", "parts2"):
        groups = PARTS4_GROUPS if (fam == "parts" and parts_vec(case)) else PARTS_GROUPS
        rows = kept_parts(case.n_part, groups, mut == "drop_group_tail")[0]
        res = {}
        for key, p, o in (("out", "part", "out0"), ("out_a", "part", "out0"), ("out_b", "part_b", "out0_b")):
            if (key == "out") == (fam == "parts"):
                res[key] = _close32(_sum32(d[p][rows], order), case.scale, case.acc, d[o], mut)
        return res
    if fam == "colsum":
        X, blocks = d["X"], block_rows(case.n_rows)
        if mut == "short_last_block":
            last = max(b for b, (a, e) in enumerate(blocks) if e > a) if case.n_rows else 0
            blocks = [(a, e - 1) if (b == last and e > a) else (a, e) for b, (a, e) in enumerate(blocks)]
        parts = np.stack([_sum32(X[a:e], order) for a, e in blocks])
        s = _sum32(X, order) if colsum_wide(case) else _sum32(parts, order)
        return {"out": _close32(s, case.scale, case.acc, d["out0"], mut), "parts": parts}
    if fam == "segs":
        res, at, any_time = {}, F32(0), False
        for k, (s, sd) in enumerate(zip(case.segs, d["segs"])):
            cols = s["col0"] + np.arange(s["len"]) * (1 if mut == "ignore_col_stride" else s["cs"])
            rows = kept_parts(s["n_part"], PARTS_GROUPS, mut == "drop_group_tail")[0]
            out = _sum32(sd["part"][rows][:, cols], order)
            if s["wrow"] and s["time_len"] > 0:
                tl, any_time = s["time_len"], True
                plain = out.copy()
                out[:s["len"] if mut == "time_scale_past" else tl] *= F32(d["t"])
                for v, w in zip((out if mut == "at_from_scaled" else plain)[:tl], sd["w"][:tl]):
                    at = F32(at + F32(v * w))
            res["out%d" % k] = out
        if any_time:
            res["at"] = float(at)
        return res
    raise KeyError(fam)
