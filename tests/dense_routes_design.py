"""Designed inputs, the float64 reference and the derived bounds for the route tests of the fp32 GroupNorm-time-GEMM kernels
of csrc/gemm.hip (test_dense_routes.py checks the design's conditions on the CPU, test_gpu_dense_routes.py runs the kernels on
it).  numpy only; nothing of the library and nothing of oracle/ is used here.

Entry points covered: gode_gn_time_gemm_f32 / _xout_f32 / _xout_aux_f32 / _pair_f32, gode_gn_time_gemm_bwd_f32, gode_wgrad_f32,
gode_group_norm_f32_fwd / _bwd and the size functions gode_gemm_bwd_parts, gode_wgrad_parts, gode_group_norm_parts.  Every
case stays below 65 536 rows, so the producer / consumer kernels of gemm_pc.hip and wgrad_split_kernel are never selected.
The limits the dispatch branches on are written out below as plain numbers (test_dense_routes.py asserts them textually
against gemm.hip); every case declares the kernel instantiation and the loop features it is meant to reach as literals, and
`route(case)` recomputes them from the numbers.

The operations.  x = sum_j c_j t_j (a fused multiply-add chain over the terms); xn = GroupNorm(x) = gamma (x - mean) rstd +
beta over groups of CG channels of a row (CG = 0: xn = x); S = t W[0] + xn W[1:]; VJP: dy = dS W[1:]^T, dx = GroupNorm'(x)^T
dy, out = out_scale dx + sum_j p_j pre_j, dgamma = sum_rows dy xhat, dbeta = sum_rows dy; weight gradient: dW[1 + i] =
sum_rows xn_i dS, dW[0] = sum_rows dS.

Two kinds of data.

`exact` - every CG = 0 route.  Terms are integers of magnitude <= 8, the coefficients powers of two with an exact 1.0 and a
0.0 among them (EXACT_COEF), t = 0.5, out_scale = -0.5, W multiples of 1/8 up to 1/2, dS and pre multiples of 1/4 up to 2.
x is a multiple of 1/4 below 82, every product x W a multiple of 1/32 with at most 12 significant bits, every product x dS a
multiple of 1/16: every partial sum in any order is a multiple of the case's granularity below 2^24 times it (exact_room: the
restatement on absolute values; for the weight gradient per partial, over the rows one block accumulates), so float32
reproduces float64 bit for bit with or without fused multiply-add and whatever the order inside the MFMA (the three bf16
pieces of the split form are exact too: x has at most 9 significant bits).  Random integers make every row and every column
different from every other, so a permuted row or column, a dropped term, a dropped time row or a skipped tile changes the
result.  Weight-gradient partials are summed by the test in float64 and compared with ==.

`real` - every route with GroupNorm.  N(0, 1) terms under tableau-like coefficients (1, then h = 0.37 times dopri5 weights of
both signs); dS is N(0, 1/16) (the older bars are absolute below 1: a cotangent of this size keeps the K-proportional bound
of the 258-column VJP under their 2e-5), pre N(0, 1).  In every group of CG >= 2 channels whose standard deviation would be below 0.75, term 0 receives an alternating
+-0.75 pattern on the side that widens it, so every group's standard deviation is >= 0.5 and rstd <= 2 (asserted on the CPU).
|gamma| in [0.5, 1.5] with both signs, beta in [-0.5, 0.5].  W = sigma s_kn max(2^(-j / 2), 2^-7), j = (k - n) mod d_in, s a random
sign, sigma = d_in^-1/2 (mod d_out where that is larger): every entry is present (the smallest moves S by 2^-7 sigma |xn|, a thousand times the bound) but the sum
of magnitudes of a row or column is 4.4 sigma instead of 0.8 d sigma, which is what keeps the K-proportional bound below under
the 1e-5 of the older tests at d = 128.  The results are compared elementwise with float64 of the same float32 inputs inside
the bounds derived now (u = 2^-24; first order in u, times 1.01 for the higher orders: every relative perturbation here is
below 2^-12).

  combine     |x~ - x| <= e_x = nterms u sum_j |c_j t_j|   (nterms fused multiply-adds; x_out and aux_out are this alone).
  stats       mean: CG - 1 additions in any order and the division: e_m = (CG - 1) u sum|x| / CG + u |m| (u |m| only where CG is
              no power of two).  The deviations d_c = x_c - m sum to zero, so the mean's error drops out of sum d^2 to first
              order; the subtraction, the square, the CG - 1 additions, the division and `+ eps` leave (CG + 4) u relative on
              v + eps, half of it on rstd, plus 3 u for rsqrt_nr ("within 1 ulp of the correctly rounded value",
              dense_common.h:16; sqrtf and the division of the generic kernel are 2 u):  rho = 3 u + (CG + 4) u / 2.
  apply       gn_apply1 (dense_common.h:54-58): scale = fl(rstd gamma), shift = fl(beta - fl(m scale)), y = fl(fl(x scale) +
              shift):  |y~ - y| <= |gamma| r (e_m + |d| (rho + u)) + u (|x sc| + |m sc| + |beta - m sc| + |y|)  at the rounded x~,
              plus what e_x does to the exact GroupNorm: d xhat_c / d x_k = r (delta_ck - (1 + xhat_c xhat_k) / CG), so
              |gamma_c| r (e_c + mean(e) + |xhat_c| mean(|xhat| e)).  Together: E_xn.
  CG = 1      mean = x exactly and rstd = eps^-1/2 = 316: the true value is beta and the true x-gradient is 0.  gn_apply1 forms
              p = fl(x scale) twice (the same bits), shift = fl(beta - p), y = fl(p + shift): |y - beta| <= u |beta - p| + u |y|
              with |p| <= 316 |gamma x| (1 + 5 u): E_xn = u (2 |beta| + 2 |p|).  No input error reaches it.
  product     a K-long accumulation in any order, fused or not: (K + 1) u sum |a| |b|; the time row adds one addend and its
              product's rounding: E_S = sum_k E_xn_k |W_kn| + (K + 1 + has_time) u (|t W_0n| + sum_k |xn_k| |W_kn|).  The split-bf16
              form adds 8 K exact piece products in K / 4 instructions (what it leaves out, lo lo, is below 2^-32 of a product);
              two roundings of the accumulator per instruction stay inside the same count.
  VJP         E_dy = (d_out + 1) u sum_n |dS_n W_in|.  dx is linear in dy: r (E_c + mean(E) + |xhat_c| mean(|xhat| E)) with
              E = |gamma| E_dy.  Through x: |d rstd| <= r^2 mean(|xhat| e), d xhat as above (xe), so |d dx_c| <= r mean(|xhat| e)
              |dx_c| + r (xe_c |m2| + |xhat_c| mean(|dh| xe)), m2 = mean(dh xhat), dh = gamma dy.  The roundings, by form:
    ATen      (gemm.hip:563-588 for CG 1 and 2, the narrow kernels, gemm.hip:1276-1287): ds = sum dh x, db = sum dh, q = db m - ds,
              c2 = q r^3 / CG, c3 = -c2 m - db r / CG, dx = r gamma dy + c2 x + c3.  e_ds = (CG + 1) u sum |dh x|, e_db = CG u sum |dh|,
              e_q = e_db |m| + |db| e_m + e_ds + 2 u |db m| + u |q|, e_c2 = r^3 / CG e_q + |c2| (3 rho + 5 u).  The same rounded c2
              multiplies x and m, so its error enters as e_c2 |x - m|:
              T1 and B carry rho + 2 u each, the products c2 x and c2 m one u, the three additions u times their operands:
              E = e_c2 |d| + |c2| e_m + r / CG e_db + (rho + 3 u) (|T1| + |B|) + 2 u c2a (|x| + |m|) + u |dx|,
              T1 = r gamma dy, B = db r / CG, c2a = |c2| + e_c2.  At CG = 1, d = 0 and e_m = 0, and T1 - B = rstd (gamma dy - dh) is
              zero under whatever rstd the kernel holds, so rho drops out: what remains is the 3 u (|T1| + |B|) = 3 u 632 |dh| of
              two products of 316 rounded apart, and e_c2 = 9.4 |dh x| only through u c2a |x|.
    normalised (the fast kernel at CG = 4, gemm.hip:557-561): dx = r (dh - m1 - xh m2): e_xh = r (e_m + u |d|) + |xhat| (rho + u),
              e_m1 = 4 u mean|dh|, e_m2 = mean(|dh| e_xh) + 5 u mean|dh xhat|,
              E = r (u |dh| + e_m1 + e_xh |m2| + |xhat| e_m2 + 3 u (|dh| + |m1| + |xhat m2|)) + |dx| (rho + u).
              out = out_scale dx + pre: |out_scale| E + u |out_scale dx| + npre u sum |p_j pre_j| + u |out|.
  reductions  over rows: a float32 accumulator sees the R rows of its block (16 rows x 4 waves, 32, or 8 rows a trip, times the
              trips of the grid-stride loop) and at most 8 more additions where lanes and waves are combined; the test adds the
              partials in float64.  (R + 8) u sum_rows |.| plus every row's own error: dgamma: E_dy |xhat| + |dy| (xe + e_xh) +
              u |dy xhat|; dbeta: E_dy; dW: E_xn |dS| with a product's u inside the (R + 8); the time row: (R + 8) u sum |dS|.

No bound is measured from the kernels.  test_dense_routes.py restates every formula in numpy float32 under four summation
orders (forward, reverse, pairwise, blocks of four) and asserts that each stays inside, and that no bound is looser than the
bar tests/test_gpu_kernels.py applies to the same quantity at the same channels per group (old_bar).
"""
import functools
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
HIGHER = 1.01

# ---- the limits the routes branch on (graph_odenet_amd/csrc/gemm.hip; line numbers of that file) --------------------------
MAX_BLOCKS = 512          # :31 `constexpr int kMaxBlocks = 512;`
TILE = 16                 # :251, :511, :964 ... `(n_rows + 15) / 16`: rows of a forward / VJP / narrow tile
WAVES = 4                 # :253, :516, :965 `blockIdx.x * 4 + wave`: 256 threads, one tile per wave and trip
WG_TILE = 32              # :642 `constexpr int R = 32;` rows of a weight-gradient tile (one per block and trip)
GEN_RB = 8                # :1173 `constexpr int RB = 8;` rows per block pass of the generic kernels
GEN_MAX_BLOCKS = 2048     # :1607, :1650, :1713, :1825 `if (blocks > 2048) blocks = 2048;`
SPLIT_MAX_BLOCKS = 256    # :1550 split-bf16 forward: 512 threads, 8 tiles a trip, at most 256 blocks
SPLIT_WAVES = 8
FAST_D = (16, 32, 64, 128)            # :1358, :1369
FAST_CG = (1, 2, 4)                   # :1362, :1373
NARROW_D_OUT = 2                      # :1368
AUX_D = 128                           # :1537 `if (aux_out && !(cg >= 0 && al && d_in == 128)) return GODE_E_UNSUPPORTED;`
MAX_TERMS = 8                         # include/graphode.h GODE_MAX_TERMS
MAX_D_IN, MAX_D_OUT = 2048, 65536     # :1426
PC_MIN_ROWS = 65536                   # :32 kWgradSplitMinRows: below it no producer / consumer kernel, no wgrad_split_kernel
LDS_ATTR = 64 * 1024                  # :1394 dynamic LDS above it needs the function attribute
E_NULLPTR, E_SHAPE, E_ALIGN, E_RANGE, E_UNSUPPORTED = -1, -2, -3, -4, -5
EPS = 1e-5
# 16-byte conditions: forward (:1535) every term, S, W, gamma, beta (x_out, aux_out misaligned: GODE_E_ALIGN, :1523-1524); pair
# (:1627) also Sb, Wb, x_out; VJP (:1671) every term of x and pre, dS, dx, gamma, both partial buffers; weight gradient (:1766)
# every term, dS, gamma, beta.  gemm_split (:1547): fast && d_in == 128 && !x_out && (split == 1 || (split == 2 && n <= 2 terms &&
# n_rows >= 65536)).


def ceil_div(a, b):
    return -(-a // b)


def fwd_blocks(n):
    return max(1, min(ceil_div(ceil_div(n, TILE), WAVES), MAX_BLOCKS))


def wgrad_blocks(n):
    return max(1, min(ceil_div(n, WG_TILE), MAX_BLOCKS))


def gen_blocks(n):
    return max(1, min(ceil_div(n, GEN_RB), GEN_MAX_BLOCKS))


def bwd_parts(n):
    return max(fwd_blocks(n), gen_blocks(n))


def split_blocks(n):
    return max(1, min(ceil_div(ceil_div(n, TILE), SPLIT_WAVES), SPLIT_MAX_BLOCKS))


def fast_cg(d_in, d_out, groups):
    if d_in != d_out or d_in not in FAST_D:
        return -1
    if groups == 0:
        return 0
    cg = d_in // groups
    return cg if (d_in % groups == 0 and cg in FAST_CG) else -1


def narrow_cg(d_in, d_out, groups):
    if d_out != NARROW_D_OUT or d_in not in FAST_D:
        return -1
    if groups == 0:
        return 0
    cg = d_in // groups
    return cg if (d_in % groups == 0 and cg in FAST_CG) else -1


def gen_fwd_lds(d_in, groups):
    return (GEN_RB * d_in + GEN_RB * max(groups, 1) * 2) * 4                 # :1605


def gen_bwd_lds(d_in, groups):
    return (GEN_RB * d_in * 2 + GEN_RB * max(groups, 1) * 2 * 2) * 4         # :1710-1711


def partition(rows_per_tile, tiles_per_trip, blocks, n):
    """Row indices each block visits: tile b * tiles_per_trip + w + k * blocks * tiles_per_trip (every trip k, every w)."""
    n_tiles = ceil_div(n, rows_per_tile)
    out = []
    for b in range(blocks):
        tiles = [t for k in range(ceil_div(n_tiles, blocks * tiles_per_trip) + 1) for t in
                 range((k * blocks + b) * tiles_per_trip, (k * blocks + b + 1) * tiles_per_trip) if t < n_tiles]
        idx = [np.arange(t * rows_per_tile, min((t + 1) * rows_per_tile, n)) for t in tiles]
        out.append(np.concatenate(idx) if idx else np.zeros(0, np.int64))
    return out


class Case:
    def __init__(self, family, name, reaches, **kw):
        self.family, self.name, self.reaches = family, name, frozenset(reaches)
        self.nterms, self.has_time, self.gamma_null, self.mis, self.xout, self.aux, self.split = 2, 1, False, None, False, False, False
        self.npre, self.out_scale, self.identity = 0, 1.0, False
        self.__dict__.update(kw)

    @property
    def cg(self):
        return self.d_in // self.groups if self.groups else 0

    @property
    def kinds(self):
        return ("exact",) if self.groups == 0 else ("real",)

    def route(self):
        return frozenset(ROUTERS[self.family](self))

    @property
    def id(self):
        return "%s/%s" % (self.family, self.name)

    def __repr__(self):
        return self.id

    def __hash__(self):
        return hash(self.id)

    def __eq__(self, other):
        return isinstance(other, Case) and self.id == other.id


# ---- routes, from the numbers above --------------------------------------------------------------------------------------
def _grid(kern, c):
    """(rows per tile, tiles per block and trip, blocks) of the kernel family `kern` at the case's size."""
    n = c.n
    if kern in ("fwd", "aux", "pair", "bwd", "nfwd", "nbwd"):
        return TILE, WAVES, fwd_blocks(n)
    if kern == "split":
        return TILE, SPLIT_WAVES, split_blocks(n)
    if kern == "wg":
        return WG_TILE, 1, wgrad_blocks(n)
    if kern == "nwg":
        return TILE, WAVES, wgrad_blocks(n)
    if kern == "gwg":
        return GEN_RB, 1, wgrad_blocks(n)
    return GEN_RB, 1, gen_blocks(n)                                        # gfwd, gbwd


def _loop_tags(kern, c):
    rows, per, blocks = _grid(kern, c)
    tags = set()
    if c.n % rows:
        tags.add(kern + ":ragged")
    if ceil_div(c.n, rows) > per * blocks:
        tags.add(kern + ":trip2")
    return tags


def trips(kern, c):
    rows, per, blocks = _grid(kern, c)
    return max(1, ceil_div(ceil_div(c.n, rows), per * blocks))


def first_trip_rows(kern, c):
    rows, per, blocks = _grid(kern, c)
    return rows * per * blocks


def _flags(c, kern=None):
    tags = set()
    if not c.has_time and kern:
        tags.add(kern + ":no_time")
    if c.gamma_null and c.groups:
        tags.add("gamma_null")
    if c.mis:
        tags.add("misaligned:" + c.mis)
    return tags


def fwd_kernel(c):
    cg, al = fast_cg(c.d_in, c.d_out, c.groups), not c.mis
    if c.aux:
        assert cg >= 0 and al and c.d_in == AUX_D
        return "aux", "aux<8,%d>" % cg
    if cg >= 0 and al and c.d_in == 128 and not c.xout and c.split:
        return "split", "split<%d,%d>" % (cg, c.nterms if c.nterms <= 2 else 0)
    if cg >= 0 and al:
        return "fwd", "fwd<%d,%d>" % (c.d_in // 16, cg)
    ncg = narrow_cg(c.d_in, c.d_out, c.groups)
    if ncg >= 0 and al:
        return "nfwd", "nfwd<%d,%d>" % (c.d_in // 16, ncg)
    return "gfwd", "gfwd:W"


def fwd_route(c):
    kern, inst = fwd_kernel(c)
    tags = {inst, "%s:terms%d" % (kern, c.nterms)} | _loop_tags(kern, c) | _flags(c, kern)
    if kern in ("fwd", "aux") and kern + ":trip2" in tags:                  # :314-315 the prefetch chain's later pairs
        if c.nterms > 4:
            tags.add(kern + ":n>4")
        if c.nterms > 6:
            tags.add(kern + ":n>6")
    if c.xout:
        tags.add(kern + ":xout")
    return tags


def pair_route(c):
    cg = fast_cg(c.d_in, c.d_in, c.groups)
    if cg >= 0 and not c.mis:
        tags = {"pair<%d,%d>" % (c.d_in // 16, cg)} | _loop_tags("pair", c)
    else:
        tags = {"pair:two_calls"}
    if c.xout:
        tags.add("pair:xout")
    return tags | _flags(c, "pair")


def bwd_kernel(c):
    cg, al = fast_cg(c.d_in, c.d_out, c.groups), not c.mis
    if cg >= 0 and al:
        return "bwd", "bwd<%d,%d>" % (c.d_in // 16, cg)
    ncg = narrow_cg(c.d_in, c.d_out, c.groups)
    if ncg >= 0 and al:
        return "nbwd", "nbwd<%d,%d>" % (c.d_in // 16, ncg)
    return "gbwd", "gbwd:W"


def bwd_route(c):
    kern, inst = bwd_kernel(c)
    tags = {inst, "%s:terms%d" % (kern, c.nterms)} | _loop_tags(kern, c) | _flags(c, kern)
    if c.groups and kern != "gbwd" and bwd_parts(c.n) > fwd_blocks(c.n):    # :623, :1091 rows of the partial buffers no block owns
        tags.add(kern + ":unowned")
    if kern == "gbwd" and gen_bwd_lds(c.d_in, c.groups) > LDS_ATTR:
        tags.add("gbwd:lds>64K")
    if c.npre:
        tags.add(kern + ":pre")
    return tags


def wgrad_kernel(c):
    cg, al = fast_cg(c.d_in, c.d_out, c.groups), not c.mis
    if cg >= 0 and al:
        return "wg", "wg<%d,%d>" % (c.d_in // 16, cg)
    ncg = narrow_cg(c.d_in, c.d_out, c.groups)
    if ncg >= 0 and al:
        return "nwg", "nwg<%d,%d>" % (c.d_in // 16, ncg)
    return "gwg", "gwg"


def wgrad_route(c):
    kern, inst = wgrad_kernel(c)
    tags = {inst, "%s:terms%d" % (kern, c.nterms)} | _loop_tags(kern, c) | _flags(c, kern)
    if c.n == 0:
        tags.add(kern + ":empty")
    return tags


def gn_route(c):
    return {"gfwd:noW", "gbwd:noW"} | {k.replace("gfwd", p) for p in ("gfwd:noW", "gbwd:noW") for k in _loop_tags("gfwd", c)} | _flags(c)


ROUTERS = {"fwd": fwd_route, "pair": pair_route, "bwd": bwd_route, "wgrad": wgrad_route, "gn": gn_route}
NJ_CG = [(nj, cg) for nj in (1, 2, 4, 8) for cg in (0, 1, 2, 4)]

# every tag some case has to reach
ROUTE_TABLE = {
    "fwd": ["fwd<%d,%d>" % p for p in NJ_CG] + ["nfwd<%d,%d>" % p for p in NJ_CG] + ["aux<8,%d>" % cg for cg in (0, 1, 2, 4)] +
           ["split<%d,%d>" % (cg, nx) for cg in (0, 1, 2, 4) for nx in (1, 2, 0)] + ["gfwd:W"] +
           ["%s:%s" % (k, f) for k in ("fwd", "aux", "split", "nfwd", "gfwd") for f in ("ragged", "trip2", "no_time")] +
           ["fwd:n>4", "fwd:n>6", "aux:n>4", "aux:n>6", "fwd:xout", "aux:xout", "nfwd:xout", "gfwd:xout", "gamma_null",
            "misaligned:x0", "misaligned:S"] + ["%s:terms%d" % (k, j) for k in ("fwd", "nfwd", "gfwd", "aux") for j in range(1, 9)] +
           ["split:terms%d" % j for j in (1, 2, 3, 5)],
    "pair": ["pair<%d,%d>" % p for p in NJ_CG] + ["pair:two_calls", "pair:ragged", "pair:trip2", "pair:xout", "pair:no_time", "gamma_null", "misaligned:x0"],
    "bwd": ["bwd<%d,%d>" % p for p in NJ_CG] + ["nbwd<%d,%d>" % p for p in NJ_CG] + ["gbwd:W"] +
           ["%s:%s" % (k, f) for k in ("bwd", "nbwd", "gbwd") for f in ("ragged", "trip2", "pre", "no_time")] +
           ["bwd:unowned", "nbwd:unowned", "gbwd:lds>64K", "gamma_null", "misaligned:x0", "misaligned:dS", "misaligned:dx"] +
           ["%s:terms%d" % (k, j) for k in ("bwd", "nbwd", "gbwd") for j in range(1, 9)],
    "wgrad": ["wg<%d,%d>" % p for p in NJ_CG] + ["nwg<%d,%d>" % p for p in NJ_CG] + ["gwg"] +
             ["%s:%s" % (k, f) for k in ("wg", "nwg", "gwg") for f in ("ragged", "trip2", "empty", "no_time")] +
             ["gamma_null", "misaligned:x0", "misaligned:dS"] +
             ["%s:terms%d" % (k, j) for k in ("wg", "nwg", "gwg") for j in range(1, 9)],
    "gn": ["gfwd:noW", "gbwd:noW", "gfwd:noW:ragged", "gfwd:noW:trip2", "gbwd:noW:ragged", "gbwd:noW:trip2", "gamma_null"],
}

# ---- cases ---------------------------------------------------------------------------------------------------------------
SWEEP_N = 37              # two full 16-row tiles and a ragged one
TILE_EDGES = (1, 15, 16, 17, 63, 64, 65)
WG_EDGES = (0, 31, 32, 33)
TRIP2_N = 32789           # MAX_BLOCKS * WAVES * TILE + 21: a full tile and a ragged one (5 rows) into the second trip
TRIP2_WG_N = 16417        # MAX_BLOCKS * WG_TILE + 33 and GEN_MAX_BLOCKS * GEN_RB + 33: a full tile and a ragged one


def _groups(d, cg):
    return d // cg if cg else 0


def _case(family, name, inst, d_in, d_out, groups, n, nterms, feats="", flags="", **kw):
    """inst: the kernel instantiation, e.g. "fwd<2,1>"; feats: its loop features; flags: tags that stand for themselves."""
    kern = inst.split("<")[0].split(":")[0]
    tags = {inst} | {"%s:%s" % (kern, f) for f in feats.split()} | set(flags.split())
    if family in ("fwd", "bwd", "wgrad"):
        tags.add("%s:terms%d" % (kern, nterms))
    return Case(family, name, tags, d_in=d_in, d_out=d_out, groups=groups, n=n, nterms=nterms, **kw)


FWD_CASES, PAIR_CASES, BWD_CASES, WGRAD_CASES, GN_CASES = [], [], [], [], []
# One channel per group makes xn = beta and dx = 0 on every row whatever x is, two make xhat = +-1 and dx = 0: such a case cannot
# see a misread row (CG 1) or a misread term (CG 1 and 2) unless it carries x_out.  So every case whose purpose is a term
# count, a tile edge or the second trip runs at CG 0 or 4 (5 on the generic kernels), and test_dense_routes.py counts a term
# or loop tag only from the cases that sees_terms / sees_rows name.  The instantiation sweep, one row per (NJ, CG):
#        NJ CG terms has_time x_out(square forward; the narrow forward takes the other) pre-terms of the VJP
SWEEP = ((1, 0, 2, 1, 0, 0), (1, 1, 3, 1, 1, 1), (1, 2, 1, 1, 0, 2), (1, 4, 5, 0, 1, 0),
         (2, 0, 7, 0, 0, 1), (2, 1, 2, 1, 1, 2), (2, 2, 4, 0, 0, 0), (2, 4, 8, 1, 1, 1),
         (4, 0, 5, 0, 0, 2), (4, 1, 1, 1, 1, 0), (4, 2, 3, 1, 0, 1), (4, 4, 6, 1, 1, 2),
         (8, 0, 8, 1, 0, 0), (8, 1, 4, 0, 1, 1), (8, 2, 2, 1, 0, 2), (8, 4, 7, 1, 1, 0))
SWEEP_GAMMA_NULL = (2, 2)
for _nj, _cg, _nt, _ht, _xo, _np in SWEEP:                                  # n = 37
    _d, _g = 16 * _nj, _groups(16 * _nj, _cg)
    _x = dict(has_time=_ht, gamma_null=(_nj, _cg) == SWEEP_GAMMA_NULL)
    _nf, _gf = ("" if _ht else " no_time"), ("gamma_null" if _x["gamma_null"] else "")
    FWD_CASES.append(_case("fwd", "sweep_d%d_cg%d" % (_d, _cg), "fwd<%d,%d>" % (_nj, _cg), _d, _d, _g, SWEEP_N, _nt, "ragged" + (" xout" if _xo else "") + _nf,
                           _gf, xout=bool(_xo), **_x))
    FWD_CASES.append(_case("fwd", "narrow_d%d_cg%d" % (_d, _cg), "nfwd<%d,%d>" % (_nj, _cg), _d, 2, _g, SWEEP_N, _nt, "ragged" + ("" if _xo else " xout") + _nf,
                           _gf, xout=not _xo, **_x))
    PAIR_CASES.append(_case("pair", "sweep_d%d_cg%d" % (_d, _cg), "pair<%d,%d>" % (_nj, _cg), _d, _d, _g, SWEEP_N, _nt, "ragged" + (" xout" if _xo else "") + _nf,
                            _gf, xout=bool(_xo), **_x))
    _p = dict(npre=_np, out_scale=-0.5 if _np else 1.0)
    _bf = "ragged" + (" pre" if _np else "") + (" unowned" if _g else "") + _nf
    BWD_CASES.append(_case("bwd", "sweep_d%d_cg%d" % (_d, _cg), "bwd<%d,%d>" % (_nj, _cg), _d, _d, _g, SWEEP_N, _nt, _bf, _gf, **_x, **_p))
    BWD_CASES.append(_case("bwd", "narrow_d%d_cg%d" % (_d, _cg), "nbwd<%d,%d>" % (_nj, _cg), _d, 2, _g, SWEEP_N, _nt, _bf, _gf, **_x, **_p))
    WGRAD_CASES.append(_case("wgrad", "sweep_d%d_cg%d" % (_d, _cg), "wg<%d,%d>" % (_nj, _cg), _d, _d, _g, SWEEP_N, _nt, "ragged" + _nf, _gf, **_x))
    WGRAD_CASES.append(_case("wgrad", "narrow_d%d_cg%d" % (_d, _cg), "nwg<%d,%d>" % (_nj, _cg), _d, 2, _g, SWEEP_N, _nt, "ragged" + _nf, _gf, **_x))
# AUX and the split-bf16 form at d = 128:  CG, AUX terms, AUX x_out, AUX has_time, split terms (third: NX = 0), split has_time
for _cg, _at, _axo, _aht, _st, _sht in ((0, 4, 0, 1, 3, 1), (1, 1, 1, 1, 5, 1), (2, 8, 0, 0, 3, 1), (4, 3, 1, 1, 5, 0)):
    FWD_CASES.append(_case("fwd", "aux_cg%d" % _cg, "aux<8,%d>" % _cg, 128, 128, _groups(128, _cg), SWEEP_N, _at,
                           "ragged" + (" xout" if _axo else "") + ("" if _aht else " no_time"), aux=True, xout=bool(_axo), has_time=_aht))
    for _nt in (1, 2, _st):
        FWD_CASES.append(_case("fwd", "split_cg%d_terms%d" % (_cg, _nt), "split<%d,%d>" % (_cg, _nt if _nt <= 2 else 0), 128, 128, _groups(128, _cg),
                               SWEEP_N, _nt, "ragged" + ("" if _sht else " no_time"), split=True, has_time=_sht))
for _n in TILE_EDGES:                                                       # tile edges at four channels per group, x_out and pre on the narrow kernels
    _r = "ragged" if _n % 16 else ""
    _u = " unowned" if bwd_parts(_n) > fwd_blocks(_n) else ""
    FWD_CASES.append(_case("fwd", "edge_n%d" % _n, "fwd<2,4>", 32, 32, 8, _n, 3, _r))
    FWD_CASES.append(_case("fwd", "narrow_edge_n%d" % _n, "nfwd<1,4>", 16, 2, 4, _n, 3, _r + " xout", xout=True))
    BWD_CASES.append(_case("bwd", "edge_n%d" % _n, "bwd<2,4>", 32, 32, 8, _n, 3, _r + _u))
    BWD_CASES.append(_case("bwd", "narrow_edge_n%d" % _n, "nbwd<1,4>", 16, 2, 4, _n, 3, _r + _u + " pre", npre=1, out_scale=-0.5))
for _n in WG_EDGES:
    _e = " empty" if _n == 0 else ""
    WGRAD_CASES.append(_case("wgrad", "edge_n%d" % _n, "wg<2,4>", 32, 32, 8, _n, 3, ("ragged" if _n % 32 else "") + _e))
    WGRAD_CASES.append(_case("wgrad", "narrow_edge_n%d" % _n, "nwg<1,4>", 16, 2, 4, _n, 3, ("ragged" if _n % 16 else "") + _e))
    WGRAD_CASES.append(_case("wgrad", "generic_edge_n%d" % _n, "gwg", 40, 40, 8, _n, 3, ("ragged" if _n % 8 else "") + (" trip2" if _n > 8 else "") + _e))
for _k in range(1, 9):                                                      # the second trips at d = 16, 1 .. 8 terms: CG 4 (even counts) and 0
    _cg = 0 if _k % 2 else 4                                                # (the VJP reads x through GroupNorm alone: CG 4 throughout)
    _f = "ragged trip2" + (" n>4" if _k > 4 else "") + (" n>6" if _k > 6 else "")
    FWD_CASES.append(_case("fwd", "trip2_d16_terms%d" % _k, "fwd<1,%d>" % _cg, 16, 16, _groups(16, _cg), TRIP2_N, _k, _f + (" xout" if _k % 2 else ""), xout=bool(_k % 2)))
    BWD_CASES.append(_case("bwd", "trip2_d16_terms%d" % _k, "bwd<1,4>", 16, 16, 4, TRIP2_N, _k, "ragged trip2 unowned"))
    WGRAD_CASES.append(_case("wgrad", "trip2_d16_terms%d" % _k, "wg<1,%d>" % _cg, 16, 16, _groups(16, _cg), TRIP2_WG_N, _k, "ragged trip2"))
# ... and once per NJ otherwise:  NJ, terms, forward (CG, x_out, has_time), VJP (CG, has_time), weight gradient (CG, has_time)
for _nj, _nt, (_fc, _fx, _fh), (_bc, _bh), (_wc, _wh) in ((2, 5, (4, 0, 0), (4, 1), (4, 0)), (4, 3, (2, 1, 1), (4, 0), (2, 1)), (8, 7, (4, 0, 1), (4, 1), (4, 1))):
    _d = 16 * _nj
    _f = "ragged trip2" + (" n>4" if _nt > 4 else "") + (" n>6" if _nt > 6 else "")
    FWD_CASES.append(_case("fwd", "trip2_d%d" % _d, "fwd<%d,%d>" % (_nj, _fc), _d, _d, _d // _fc, TRIP2_N, _nt, _f + (" xout" if _fx else "") + ("" if _fh else " no_time"),
                           xout=bool(_fx), has_time=_fh))
    BWD_CASES.append(_case("bwd", "trip2_d%d" % _d, "bwd<%d,%d>" % (_nj, _bc), _d, _d, _d // _bc, TRIP2_N, _nt, "ragged trip2 unowned pre" + ("" if _bh else " no_time"),
                           npre=1, out_scale=-0.5, has_time=_bh))
    WGRAD_CASES.append(_case("wgrad", "trip2_d%d" % _d, "wg<%d,%d>" % (_nj, _wc), _d, _d, _d // _wc, TRIP2_WG_N, _nt, "ragged trip2" + ("" if _wh else " no_time"), has_time=_wh))
    WGRAD_CASES.append(_case("wgrad", "trip2_d%d_exact" % _d, "wg<%d,0>" % _nj, _d, _d, 0, TRIP2_WG_N, _nt, "ragged trip2"))     # the reduction over rows, bit for bit
FWD_CASES += [
    _case("fwd", "aux_trip2", "aux<8,4>", 128, 128, 32, TRIP2_N, 7, "ragged trip2 n>4 n>6 xout", aux=True, xout=True),
    _case("fwd", "split_trip2", "split<4,2>", 128, 128, 32, TRIP2_N, 2, "ragged trip2", split=True),
    _case("fwd", "narrow_trip2", "nfwd<1,4>", 16, 2, 4, TRIP2_N, 6, "ragged trip2"),
    _case("fwd", "generic_trip2", "gfwd:W", 16, 34, 4, TRIP2_WG_N, 4, "ragged trip2 xout", xout=True),
    _case("fwd", "generic_d24", "gfwd:W", 24, 24, 24, SWEEP_N, 2, "ragged"),
    _case("fwd", "generic_d40", "gfwd:W", 40, 40, 8, SWEEP_N, 5, "ragged"),
    _case("fwd", "generic_d96", "gfwd:W", 96, 96, 32, SWEEP_N, 7, "ragged"),
    _case("fwd", "generic_d64_cg8", "gfwd:W", 64, 64, 8, SWEEP_N, 1, "ragged"),
    _case("fwd", "generic_d128_cg16", "gfwd:W", 128, 128, 8, SWEEP_N, 8, "ragged"),
    _case("fwd", "generic_16x34", "gfwd:W", 16, 34, 16, SWEEP_N, 3, "ragged"),
    _case("fwd", "generic_128x258", "gfwd:W", 128, 258, 32, SWEEP_N, 6, "ragged no_time", has_time=0),
    _case("fwd", "generic_24x7", "gfwd:W", 24, 7, 0, SWEEP_N, 2, "ragged"),
    _case("fwd", "generic_2048x3", "gfwd:W", 2048, 3, 0, 9, 2, "ragged"),
    _case("fwd", "mis_x0", "gfwd:W", 32, 32, 8, SWEEP_N, 2, "ragged", "misaligned:x0", mis="x0"),
    _case("fwd", "mis_S", "gfwd:W", 32, 32, 0, SWEEP_N, 2, "ragged", "misaligned:S", mis="S"),
]
for _k in (2, 3, 4, 5, 6, 7):                                               # the remaining term counts of the AUX chain
    FWD_CASES.append(_case("fwd", "aux_terms%d" % _k, "aux<8,4>", 128, 128, 32, 17, _k, "ragged", aux=True))
for _k in range(1, 9):                                                      # 1 .. 8 terms on the narrow and generic kernels, where x is seen
    FWD_CASES.append(_case("fwd", "narrow_terms%d" % _k, "nfwd<1,4>", 16, 2, 4, 17, _k, "ragged"))
    FWD_CASES.append(_case("fwd", "generic_terms%d" % _k, "gfwd:W", 40, 40, 8, 9, _k, "ragged"))
    BWD_CASES.append(_case("bwd", "narrow_terms%d" % _k, "nbwd<1,4>", 16, 2, 4, 17, _k, "ragged unowned"))
    BWD_CASES.append(_case("bwd", "generic_terms%d" % _k, "gbwd:W", 40, 40, 8, 9, _k, "ragged"))
    WGRAD_CASES.append(_case("wgrad", "narrow_terms%d" % _k, "nwg<1,4>", 16, 2, 4, 17, _k, "ragged"))
    WGRAD_CASES.append(_case("wgrad", "generic_terms%d" % _k, "gwg", 40, 40, 8, 9, _k, "ragged trip2"))
PAIR_CASES += [
    _case("pair", "trip2", "pair<1,4>", 16, 16, 4, TRIP2_N, 3, "ragged trip2"),
    _case("pair", "full_tiles", "pair<2,4>", 32, 32, 8, 64, 2, ""),
    _case("pair", "two_calls_d24", "pair:two_calls", 24, 24, 24, SWEEP_N, 2, "xout", xout=True),
    _case("pair", "two_calls_mis_x0", "pair:two_calls", 32, 32, 8, SWEEP_N, 2, "", "misaligned:x0", mis="x0"),
]
BWD_CASES += [
    _case("bwd", "narrow_trip2", "nbwd<1,4>", 16, 2, 4, TRIP2_N, 6, "ragged trip2 unowned pre", npre=1),
    _case("bwd", "generic_trip2", "gbwd:W", 16, 34, 4, TRIP2_WG_N, 4, "ragged trip2"),
    _case("bwd", "generic_d24", "gbwd:W", 24, 24, 24, SWEEP_N, 2, "ragged pre", npre=2, out_scale=-0.5),
    _case("bwd", "generic_d40", "gbwd:W", 40, 40, 8, SWEEP_N, 5, "ragged"),
    _case("bwd", "generic_d96", "gbwd:W", 96, 96, 32, SWEEP_N, 7, "ragged", "gamma_null", gamma_null=True),
    _case("bwd", "generic_d64_cg8", "gbwd:W", 64, 64, 8, SWEEP_N, 1, "ragged"),
    _case("bwd", "generic_d128_cg16", "gbwd:W", 128, 128, 8, SWEEP_N, 8, "ragged pre", npre=1),
    _case("bwd", "generic_16x34", "gbwd:W", 16, 34, 16, SWEEP_N, 3, "ragged"),
    _case("bwd", "generic_128x258", "gbwd:W", 128, 258, 32, SWEEP_N, 6, "ragged no_time", has_time=0),
    _case("bwd", "generic_24x7", "gbwd:W", 24, 7, 0, SWEEP_N, 2, "ragged pre", npre=1, out_scale=-0.5),
    _case("bwd", "generic_2048x3", "gbwd:W", 2048, 3, 0, 9, 2, "ragged lds>64K"),
    _case("bwd", "mis_x0", "gbwd:W", 32, 32, 8, SWEEP_N, 2, "ragged", "misaligned:x0", mis="x0"),
    _case("bwd", "mis_dS", "gbwd:W", 32, 32, 0, SWEEP_N, 2, "ragged", "misaligned:dS", mis="dS"),
    _case("bwd", "mis_dx", "gbwd:W", 32, 32, 8, SWEEP_N, 2, "ragged", "misaligned:dx", mis="dx"),
]
WGRAD_CASES += [
    _case("wgrad", "narrow_trip2", "nwg<1,4>", 16, 2, 4, TRIP2_N, 6, "ragged trip2"),
    _case("wgrad", "generic_trip2", "gwg", 16, 34, 4, TRIP2_WG_N, 4, "ragged trip2"),
    _case("wgrad", "generic_d24", "gwg", 24, 24, 24, SWEEP_N, 3, "ragged trip2"),
    _case("wgrad", "generic_d40", "gwg", 40, 40, 8, SWEEP_N, 5, "ragged trip2"),
    _case("wgrad", "generic_d96", "gwg", 96, 96, 32, SWEEP_N, 7, "ragged trip2", "gamma_null", gamma_null=True),
    _case("wgrad", "generic_d64_cg8", "gwg", 64, 64, 8, SWEEP_N, 1, "ragged trip2"),
    _case("wgrad", "generic_d128_cg16", "gwg", 128, 128, 8, SWEEP_N, 8, "ragged trip2"),
    _case("wgrad", "generic_16x34", "gwg", 16, 34, 16, SWEEP_N, 2, "ragged trip2"),
    _case("wgrad", "generic_128x258", "gwg", 128, 258, 32, SWEEP_N, 6, "ragged trip2 no_time", has_time=0),
    _case("wgrad", "generic_24x7", "gwg", 24, 7, 0, SWEEP_N, 2, "ragged trip2"),
    _case("wgrad", "generic_2048x3", "gwg", 2048, 3, 0, 9, 2, "ragged trip2"),
    _case("wgrad", "mis_x0", "gwg", 32, 32, 8, SWEEP_N, 2, "ragged trip2", "misaligned:x0", mis="x0"),
    _case("wgrad", "mis_dS", "gwg", 32, 32, 0, SWEEP_N, 2, "ragged trip2", "misaligned:dS", mis="dS"),
]


def _gn(name, d, groups, n, feats, flags="", **kw):
    tags = {"gfwd:noW", "gbwd:noW"} | {"%s:%s" % (k, f) for k in ("gfwd:noW", "gbwd:noW") for f in feats.split()} | set(flags.split())
    return Case("gn", name, tags, d_in=d, d_out=d, groups=groups, n=n, nterms=1, has_time=0, **kw)


GN_CASES += [_gn("d24_g24", 24, 24, SWEEP_N, "ragged"), _gn("d40_g8", 40, 8, SWEEP_N, "ragged"), _gn("d96_g32", 96, 32, 64, "", "gamma_null", gamma_null=True),
             _gn("d128_g32", 128, 32, SWEEP_N, "ragged"), _gn("d7_g1", 7, 1, 5, "ragged"), _gn("trip2", 16, 4, TRIP2_WG_N, "ragged trip2")]

FAMILIES = {"fwd": FWD_CASES, "pair": PAIR_CASES, "bwd": BWD_CASES, "wgrad": WGRAD_CASES, "gn": GN_CASES}
ALL_CASES = [c for cases in FAMILIES.values() for c in cases]
BY_ID = {c.id: c for c in ALL_CASES}
LARGE_N = 4200            # cases from here on are the second trips

# ---- data ----------------------------------------------------------------------------------------------------------------
EXACT_COEF = (1.0, -0.5, 2.0, 0.0, 0.25, -4.0, 0.5, -2.0)
EXACT_AUX_COEF = (0.5, 1.0, -2.0, 0.25, 0.0, 2.0, -0.5, 4.0)
H = 0.37
REAL_COEF = (1.0, H * 35 / 384, -H * 2187 / 6784, H * 500 / 1113, H * 125 / 192, -H * 0.0123, H * 11 / 84, -H * 1.7)
REAL_AUX_COEF = (1.0, H * 5179 / 57600, -H * 7571 / 16695, H * 393 / 640, -H * 92097 / 339200, H * 187 / 2100, H / 40, H * 0.9)
EXACT_PRE_COEF, REAL_PRE_COEF = (1.0, -0.5), (1.0, H / 6)
EXACT_T, REAL_T = 0.5, 0.37
MIN_STD, WIDEN = 0.5, 0.75
W_FLOOR = 2.0 ** -7
REAL_DS_STD = 0.25


def _rng(case, kind):
    return np.random.RandomState(zlib.crc32(("%s/%s" % (case.id, kind)).encode()))


def _weights(rng, k_rows, d_in, d_out, kind):
    """(has_time + d_in) x d_out: exact - multiples of 1/8 up to 1/2; real - the decaying magnitudes of the module docstring."""
    if kind == "exact":
        return (rng.randint(-4, 5, (k_rows, d_out)) / 8.0).astype(F32)
    j = (np.arange(d_in)[:, None] - np.arange(d_out)[None, :]) % max(d_in, d_out)
    w1 = np.maximum(2.0 ** (-j / 2.0), W_FLOOR) * rng.choice((-1.0, 1.0), (d_in, d_out)) / np.sqrt(d_in)
    w0 = rng.standard_normal((k_rows - d_in, d_out)) / np.sqrt(d_in)
    return np.concatenate([w0, w1]).astype(F32)


def combine64(coef, terms):
    x = sum((F64(c) * t.astype(F64) for c, t in zip(coef, terms)), np.zeros(terms[0].shape))
    reach = sum((abs(F64(c)) * np.abs(t.astype(F64)) for c, t in zip(coef, terms)), np.zeros(terms[0].shape))
    return x, reach


def _widen(case, coef, terms):
    """real data: every group of CG >= 2 channels gets a standard deviation >= WIDEN where it was below (module docstring)."""
    cg = case.cg
    if cg < 2 or case.n == 0:
        return
    x, _ = combine64(coef, terms)
    g = x.reshape(case.n, case.groups, cg)
    dev = g - g.mean(2, keepdims=True)
    s = np.where(np.arange(cg) % 2 == 0, 1.0, -1.0)
    if cg % 2:
        s[-1] = 0.0
    side = np.where((dev * s).sum(2, keepdims=True) >= 0, 1.0, -1.0)
    low = np.sqrt((dev ** 2).mean(2, keepdims=True)) < WIDEN
    terms[0] += (np.where(low, side * WIDEN / np.sqrt((cg - cg % 2) / cg), 0.0) * s).reshape(case.n, case.d_in).astype(F32)


@functools.lru_cache(maxsize=4)
def inputs(case, kind):
    assert kind in case.kinds
    rng, ex = _rng(case, kind), kind == "exact"
    n, d_in, d_out, k_rows = case.n, case.d_in, case.d_out, case.d_in + case.has_time
    coef = (EXACT_COEF if ex else REAL_COEF)[:case.nterms]
    if ex:
        terms = [(rng.randint(1, 9, (n, d_in)) * rng.choice((-1, 1), (n, d_in))).astype(F32) for _ in coef]
    else:
        terms = [rng.standard_normal((n, d_in)).astype(F32) for _ in coef]
        _widen(case, coef, terms)
    d = {"coef": np.array(coef, F32), "terms": terms, "t": EXACT_T if ex else REAL_T, "eps": EPS, "gamma": None, "beta": None}
    if case.groups and not case.gamma_null:
        d["gamma"] = ((rng.rand(d_in) + 0.5) * rng.choice((-1.0, 1.0), d_in)).astype(F32)
        d["beta"] = (rng.rand(d_in) - 0.5).astype(F32)
    if case.family in ("fwd", "pair", "bwd"):
        d["W"] = np.eye(d_in, dtype=F32) if case.identity else _weights(rng, k_rows, d_in, d_out, kind)
    if case.family == "pair":
        d["Wb"] = _weights(rng, k_rows, d_in, d_out, kind)
    if case.aux:
        d["aux_coef"] = np.array((EXACT_AUX_COEF if ex else REAL_AUX_COEF)[:case.nterms], F32)
    if case.family in ("bwd", "wgrad", "gn"):
        d["dS"] = (rng.randint(-8, 9, (n, d_out)) / 4.0).astype(F32) if ex else (REAL_DS_STD * rng.standard_normal((n, d_out))).astype(F32)
    if case.family == "bwd":
        d["out_scale"] = case.out_scale
        d["pre_coef"] = np.array((EXACT_PRE_COEF if ex else REAL_PRE_COEF)[:case.npre], F32)
        d["pre"] = [(rng.randint(-8, 9, (n, d_in)) / 4.0).astype(F32) if ex else rng.standard_normal((n, d_in)).astype(F32) for _ in range(case.npre)]
    return d


# ---- float64 reference (mut: one planted defect) and derived bounds: {quantity: (ref, bound)} ----------------------------
MUTATIONS = ("drop_last_term", "drop_terms_5_8", "drop_time_row", "time_not_scaled", "skip_ragged_tile", "trip2_from_trip1",
             "swap_gamma_beta", "w_untransposed", "ignore_out_scale", "ignore_pre", "pre_scaled", "aux_main_coefs", "pair_sb_with_wa",
             "neighbour_group_stats", "colsum_missing_pass")


def gn64(x, case, gamma, beta, eps, mut=None):
    """GroupNorm in float64: (xn, xhat, mean, rstd, d), each n x d_in."""
    n, d = x.shape
    if case.groups == 0:
        return x, x, np.zeros_like(x), np.ones_like(x), x
    cg = case.cg
    g = x.reshape(n, case.groups, cg)
    m = np.repeat(g.mean(2), cg, 1)
    v = np.repeat(((g - g.mean(2, keepdims=True)) ** 2).mean(2), cg, 1)
    r = 1.0 / np.sqrt(v + eps)
    if mut == "neighbour_group_stats" and case.groups > 1:                  # channel 0 of group 1 under group 0's statistics
        m, r = m.copy(), r.copy()
        m[:, cg], r[:, cg] = m[:, 0], r[:, 0]
    gam = np.ones(d) if gamma is None else gamma.astype(F64)
    bet = np.zeros(d) if beta is None else beta.astype(F64)
    if mut == "swap_gamma_beta":
        gam, bet = bet, gam
    xh = (x - m) * r
    return gam * xh + bet, xh, m, r, x - m


def _gmean(a, case):
    """Mean over each group, broadcast back to n x d_in."""
    cg = case.cg
    return np.repeat(a.reshape(a.shape[0], case.groups, cg).mean(2), cg, 1)


def gn_fwd_bound(case, x, e_x, xn, xh, m, r, dev, gamma, beta):
    """E_xn of the module docstring."""
    if case.groups == 0:
        return e_x
    cg, d = case.cg, x.shape[1]
    gam = np.ones(d) if gamma is None else np.abs(gamma.astype(F64))
    bet = np.zeros(d) if beta is None else beta.astype(F64)
    if cg == 1:
        p = r * gam * np.abs(x) * (1 + 5 * U)
        return HIGHER * U * (2 * np.abs(bet) + 2 * p)
    e_m, rho = stats_err(case, x, m)
    sc = r * gam
    rounding = gam * r * (e_m + np.abs(dev) * (rho + U)) + U * (np.abs(x) * sc + np.abs(m) * sc + np.abs(bet) + np.abs(m) * sc + np.abs(xn))
    return HIGHER * (rounding + gam * xhat_input_err(case, e_x, xh, r))


def stats_err(case, x, m):
    cg = case.cg
    pow2 = cg & (cg - 1) == 0
    e_m = (cg - 1) * U * _gmean(np.abs(x), case) + (0.0 if pow2 else U * np.abs(m))
    return e_m, 3 * U + (cg + 4) * U / 2


def xhat_input_err(case, e, xh, r):
    """What a perturbation of x within e does to xhat, to first order (the derivative of the module docstring)."""
    return r * (e + _gmean(e, case) + np.abs(xh) * _gmean(np.abs(xh) * e, case))


def bwd_form(case):
    return "normalised" if (bwd_kernel(case)[0] == "bwd" and case.cg == 4 and case.family == "bwd") else "aten"


def gn_bwd64(case, x, dy, gamma, eps, mut=None):
    """GroupNorm'(x)^T dy in float64."""
    if case.groups == 0:
        return dy
    _, xh, m, r, _ = gn64(x, case, gamma, None, eps, mut)
    gam = np.ones(x.shape[1]) if gamma is None else gamma.astype(F64)
    dh = dy * gam
    return r * (dh - _gmean(dh, case) - xh * _gmean(dh * xh, case))


def gn_bwd_bound(case, x, e_x, dy, e_dy, gamma, eps):
    """(error bound of dx, per-element error of xhat as the kernels form it) by the VJP derivation of the module docstring."""
    cg, d = case.cg, x.shape[1]
    gam = np.ones(d) if gamma is None else gamma.astype(F64)
    _, xh, m, r, dev = gn64(x, case, gamma, None, eps)
    dh, ag = dy * gam, np.abs(gam)
    dx = r * (dh - _gmean(dh, case) - xh * _gmean(dh * xh, case))
    e_m, rho = stats_err(case, x, m)
    if cg == 1:
        e_m = np.zeros_like(x)
    e_xh = r * (e_m + U * np.abs(dev)) + np.abs(xh) * (rho + U)
    # through dy (linear) and through x
    eh = ag * e_dy
    lin = r * (eh + _gmean(eh, case) + np.abs(xh) * _gmean(np.abs(xh) * eh, case))
    xe = xhat_input_err(case, e_x, xh, r)
    m2 = _gmean(dh * xh, case)
    thru_x = r * _gmean(np.abs(xh) * e_x, case) * np.abs(dx) + r * (xe * np.abs(m2) + np.abs(xh) * _gmean(np.abs(dh) * xe, case))
    if cg == 1:                                                             # xhat is (x - x) rstd = 0 whatever x is
        thru_x, xe = np.zeros_like(x), np.zeros_like(x)
    if bwd_form(case) == "normalised":
        m1 = _gmean(dh, case)
        e_m1 = 4 * U * _gmean(np.abs(dh), case)
        e_m2 = _gmean(np.abs(dh) * e_xh, case) + 5 * U * _gmean(np.abs(dh * xh), case)
        rnd = r * (U * np.abs(dh) + e_m1 + e_xh * np.abs(m2) + np.abs(xh) * e_m2 + 3 * U * (np.abs(dh) + np.abs(m1) + np.abs(xh * m2))) + np.abs(dx) * (rho + U)
    else:
        gsum = lambda a: cg * _gmean(a, case)                              # noqa: E731
        ds, db = gsum(dh * x), gsum(dh)
        e_ds, e_db = (cg + 1) * U * gsum(np.abs(dh * x)), cg * U * gsum(np.abs(dh))
        q = db * m - ds
        e_q = e_db * np.abs(m) + np.abs(db) * e_m + e_ds + 2 * U * np.abs(db * m) + U * np.abs(q)
        c2 = q * r ** 3 / cg
        e_c2 = r ** 3 / cg * e_q + np.abs(c2) * (3 * rho + 5 * U)
        c2a = np.abs(c2) + e_c2
        t1, b = np.abs(r * dh), np.abs(db * r / cg)
        rho_tb = 0.0 if cg == 1 else rho                                   # CG = 1: the one rounded rstd multiplies T1 and B, which cancel
        rnd = e_c2 * np.abs(dev) + np.abs(c2) * e_m + r / cg * e_db + (rho_tb + 3 * U) * (t1 + b) + \
            2 * U * c2a * (np.abs(x) + np.abs(m)) + U * np.abs(dx)
    return HIGHER * (lin + thru_x + rnd), xe + e_xh, xh


def _rows_acc(kern, case):
    """R of the module docstring: the rows one float32 accumulator of the reduction sees."""
    rows, per, _ = _grid(kern, case)
    return rows * per * trips(kern, case)


def _trip_mutate(case, kern, mut, arrays):
    """Row mutations of per-row outputs: the last ragged tile skipped (NaN), the second trip's rows taken from the first."""
    rows, _, _ = _grid(kern, case)
    out = []
    for a in arrays:
        a = a.copy()
        if mut == "skip_ragged_tile" and case.n % rows:
            a[case.n - case.n % rows:] = np.nan
        if mut == "trip2_from_trip1" and case.n > first_trip_rows(kern, case):
            f = first_trip_rows(kern, case)
            a[f:] = a[:case.n - f]
        out.append(a)
    return out


def _terms(d, mut):
    coef, terms = list(d["coef"]), list(d["terms"])
    if mut == "drop_last_term" and len(coef) > 1:
        coef, terms = coef[:-1], terms[:-1]
    if mut == "drop_terms_5_8":
        coef, terms = coef[:4], terms[:4]
    return coef, terms


def _fwd_parts(case, d, mut, W):
    coef, terms = _terms(d, mut)
    x, reach = combine64(coef, terms)
    e_x = case.nterms * U * reach
    xn, xh, m, r, dev = gn64(x, case, d["gamma"], d["beta"], d["eps"], mut)
    e_xn = gn_fwd_bound(case, x, e_x, xn, xh, m, r, dev, d["gamma"], d["beta"])
    W64, ht = W.astype(F64), case.has_time
    t = F64(F32(d["t"]))
    S = xn @ W64[ht:]
    reach_s = np.abs(xn) @ np.abs(W64[ht:])
    if ht and mut != "drop_time_row":
        S = S + (1.0 if mut == "time_not_scaled" else t) * W64[0]
        reach_s = reach_s + np.abs(t * W64[0])
    e_s = e_xn @ np.abs(W64[ht:]) + (case.d_in + 1 + ht) * U * reach_s
    return x, e_x, S, e_s


def reference(case, kind, mut=None):
    return _reference(case, kind, mut)


@functools.lru_cache(maxsize=4)
def _reference(case, kind, mut):
    d, fam = inputs(case, kind), case.family
    res = {}
    if fam in ("fwd", "pair"):
        kern = fwd_kernel(case)[0] if fam == "fwd" else "pair"
        x, e_x, S, e_s = _fwd_parts(case, d, mut, d["W"])
        res["S"] = (S, e_s)
        if fam == "pair":
            _, _, Sb, e_sb = _fwd_parts(case, d, mut, d["W"] if mut == "pair_sb_with_wa" else d["Wb"])
            res["Sb"] = (Sb, e_sb)
        if case.xout:
            res["xout"] = (x, e_x)
        if case.aux:
            coef, terms = _terms(dict(d, coef=d["coef"] if mut == "aux_main_coefs" else d["aux_coef"]), mut)
            a, reach = combine64(coef, terms)
            res["aux"] = (a, case.nterms * U * reach)
        keys = list(res)
        for k, a in zip(keys, _trip_mutate(case, kern, mut, [res[k][0] for k in keys])):
            res[k] = (a, res[k][1])
        return res
    if fam in ("bwd", "gn"):
        kern = bwd_kernel(case)[0] if fam == "bwd" else "gbwd"
        coef, terms = _terms(d, mut)
        x, reach = combine64(coef, terms)
        e_x = (case.nterms * U * reach) if fam == "bwd" else np.zeros_like(x)
        dS = d["dS"].astype(F64)
        if fam == "bwd":
            W1 = d["W"].astype(F64)[case.has_time:]
            dy = dS @ (W1 if (mut == "w_untransposed" and case.d_in == case.d_out) else W1.T)
            e_dy = (case.d_out + 1) * U * (np.abs(dS) @ np.abs(W1.T))
        else:
            dy, e_dy = dS, np.zeros_like(dS)
            xn, xh, m, r, dev = gn64(x, case, d["gamma"], d["beta"], d["eps"], mut)
            res["y"] = (xn, gn_fwd_bound(case, x, e_x, xn, xh, m, r, dev, d["gamma"], d["beta"]))
        dx = gn_bwd64(case, x, dy, d["gamma"], d["eps"], mut)
        if case.groups:
            e_dx, e_xh, xh = gn_bwd_bound(case, x, e_x, dy, e_dy, d["gamma"], d["eps"])
        else:
            e_dx, e_xh, xh = e_dy, None, None
        if fam == "bwd":
            sc = 1.0 if mut == "ignore_out_scale" else F64(F32(d["out_scale"]))
            pre, pre_reach = combine64(d["pre_coef"], d["pre"]) if case.npre else (np.zeros_like(x), np.zeros_like(x))
            if mut == "ignore_pre":
                pre = np.zeros_like(x)
            out = sc * (dx + pre) if mut == "pre_scaled" else sc * dx + pre
            e_out = abs(sc) * e_dx + U * np.abs(sc * dx) + case.npre * U * pre_reach + U * np.abs(out)
        else:
            out, e_out = dx, e_dx
        res["dx"] = (_trip_mutate(case, kern, mut, [out])[0], e_out)
        if case.groups:
            if mut in ("swap_gamma_beta", "neighbour_group_stats"):
                xh = gn64(x, case, d["gamma"], d["beta"], d["eps"], mut)[1]
            rows = np.ones(case.n, bool)
            if mut == "skip_ragged_tile" and case.n % _grid(kern, case)[0]:
                rows[case.n - case.n % _grid(kern, case)[0]:] = False
            R = _rows_acc(kern, case) + 8
            dg, db = (dy * xh)[rows].sum(0), dy[rows].sum(0)
            e_dg = (e_dy * np.abs(xh) + np.abs(dy) * e_xh + U * np.abs(dy * xh)).sum(0) + R * U * np.abs(dy * xh).sum(0)
            e_db = e_dy.sum(0) + R * U * np.abs(dy).sum(0)
            res["dgamma"], res["dbeta"] = (dg, HIGHER * e_dg), (db, HIGHER * e_db)
        return res
    if fam == "wgrad":
        kern = wgrad_kernel(case)[0]
        coef, terms = _terms(d, mut)
        x, reach = combine64(coef, terms)
        e_x = case.nterms * U * reach
        xn, xh, m, r, dev = gn64(x, case, d["gamma"], d["beta"], d["eps"], mut)
        e_xn = gn_fwd_bound(case, x, e_x, xn, xh, m, r, dev, d["gamma"], d["beta"])
        dS = d["dS"].astype(F64)
        rows = np.ones(case.n, bool)
        rpt = _grid(kern, case)[0]
        if mut == "skip_ragged_tile" and case.n % rpt:
            rows[case.n - case.n % rpt:] = False
        if mut == "trip2_from_trip1" and case.n > first_trip_rows(kern, case):
            f = first_trip_rows(kern, case)
            xn = xn.copy()
            xn[f:] = xn[:case.n - f]
        R = _rows_acc(kern, case) + 8
        res["dW"] = (xn[rows].T @ dS[rows], HIGHER * (e_xn.T @ np.abs(dS) + R * U * (np.abs(xn).T @ np.abs(dS))))
        if case.has_time:
            r0 = rows.copy()
            if mut == "colsum_missing_pass" and kern == "wg":
                rpp = min(WG_TILE, 256 // (case.d_in // 4))                 # :644 rows per staging pass
                r0 &= (np.arange(case.n) % WG_TILE) < WG_TILE - rpp
            if mut != "drop_time_row":
                res["dW0"] = (dS[r0].sum(0), R * U * np.abs(dS).sum(0))
            else:
                res["dW0"] = (np.zeros(case.d_out), R * U * np.abs(dS).sum(0))
        return res
    raise KeyError(fam)


def old_bar(case, quantity, ref):
    """The bar tests/test_gpu_kernels.py applies to this quantity at the case's channels per group (absolute)."""
    cg, n = case.cg, max(case.n, 1)
    scale = max(1.0, float(np.abs(ref).max(initial=0)))
    if quantity in ("S", "Sb", "y"):
        return {1: 2e-4, 2: 2e-5}.get(cg, 1e-5) * scale
    if quantity in ("xout", "aux"):
        return 1e-6 * scale
    if quantity == "dx":
        return {0: 1e-5, 1: 2e-3, 2: 1e-4}.get(cg, 2e-5) * scale
    if quantity == "dgamma":
        return (2e-3 if cg == 1 else 2e-5) * n ** 0.5 * scale
    if quantity == "dbeta":
        return 2e-5 * n ** 0.5 * scale
    if quantity == "dW":
        return max({1: 2e-4, 2: 2e-5}.get(cg, 1e-5), 2e-5) * n ** 0.5 * scale
    if quantity == "dW0":                                                   # the older tests compare t * row 0
        return 2e-5 * n ** 0.5 * max(1.0, REAL_T * float(np.abs(ref).max(initial=0))) / REAL_T
    raise KeyError(quantity)


# ---- the comparisons the GPU test uses --------------------------------------------------------------------------------------
def exact_equal(got, ref):
    """got (float32 array, or a float64 sum of float32 partials) is the float64 reference."""
    got = np.asarray(got)
    if got.shape != np.shape(ref) or np.isnan(got).any():
        return False
    return np.array_equal(got, np.asarray(ref).astype(got.dtype))


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
    """exact data: (largest partial sum on absolute values) / granularity over every accumulation of the case; below 2^24 every
    order is exact.  The weight gradient: per partial, over the rows its block visits."""
    d, fam = inputs(case, "exact"), case.family
    _, reach = combine64(d["coef"], d["terms"])
    room = reach.max(initial=0) / 0.25                                      # the combine: multiples of 1/4
    if case.aux:
        room = max(room, combine64(d["aux_coef"], d["terms"])[1].max(initial=0) / 0.25)
    if fam in ("fwd", "pair"):
        for key in ("W", "Wb")[:1 + (fam == "pair")]:
            W = np.abs(d[key].astype(F64))
            room = max(room, ((reach @ W[case.has_time:]) + (EXACT_T * W[0] if case.has_time else 0)).max(initial=0) * 32)
    if fam == "bwd":
        dy = np.abs(d["dS"].astype(F64)) @ np.abs(d["W"].astype(F64)[case.has_time:].T)
        pre = combine64(d["pre_coef"], d["pre"])[1] if case.npre else 0.0
        room = max(room, (dy.max(initial=0)) * 32, (abs(case.out_scale) * dy + pre).max(initial=0) * 64)
    if fam == "wgrad":
        kern = wgrad_kernel(case)[0]
        rows, per, blocks = _grid(kern, case)
        dS = np.abs(d["dS"].astype(F64))
        for idx in partition(rows, per, blocks, case.n):
            if idx.size:
                room = max(room, (reach[idx].T @ dS[idx]).max() * 16, dS[idx].sum(0).max() * 4)
    return float(room)


# ---- float32 restatements of the kernels under a summation order ------------------------------------------------------------
ORDERS = ("forward", "reverse", "pairwise", "blocks4")


def osum(get, length, order):
    """sum_i get(i), i < length, in float32 in the given order (get returns float32 arrays of one shape)."""
    if length == 0:
        return None
    if order == "forward" or order == "reverse":
        idx = range(length) if order == "forward" else range(length - 1, -1, -1)
        acc = None
        for i in idx:
            acc = get(i) if acc is None else acc + get(i)
        return acc
    if order == "blocks4":
        acc = None
        for i0 in range(0, length, 4):
            b = [get(i) for i in range(i0, min(i0 + 4, length))]
            s = (b[0] + b[1]) + (b[2] + b[3]) if len(b) == 4 else functools.reduce(lambda p, q: p + q, b)
            acc = s if acc is None else acc + s
        return acc

    def pair(lo, hi):
        if hi - lo == 1:
            return get(lo)
        mid = (lo + hi) // 2
        return pair(lo, mid) + pair(mid, hi)
    return pair(0, length)


def matmul32(a, b, order, init=None):
    """a (N x K) @ b (K x M) in float32: rounded products added in `order` (after `init`)."""
    s = osum(lambda k: a[:, k:k + 1] * b[k:k + 1, :], a.shape[1], order)
    if s is None:
        s = np.zeros((a.shape[0], b.shape[1]), F32)
    return s if init is None else init + s


def combine32(coef, terms):
    x = np.zeros(terms[0].shape, F32)
    for c, t in zip(coef, terms):
        x = x + F32(c) * t
    return x


def gn32(case, x, gamma, beta, eps, order):
    """float32 GroupNorm by the kernels' steps: (xn, xh, mean, rstd)."""
    n, d = x.shape
    if case.groups == 0:
        return x, x, None, None
    cg = case.cg
    g = x.reshape(n, case.groups, cg)
    if cg == 1:
        m = g[:, :, 0]
        v = np.zeros_like(m)
    else:
        m = osum(lambda c: g[:, :, c], cg, order) / F32(cg)
        v = osum(lambda c: (g[:, :, c] - m) * (g[:, :, c] - m), cg, order) / F32(cg)
    r = (F32(1) / np.sqrt(v + F32(eps))).astype(F32)
    m, r = np.repeat(m, cg, 1), np.repeat(r, cg, 1)
    gam = np.ones(d, F32) if gamma is None else gamma
    bet = np.zeros(d, F32) if beta is None else beta
    scale = r * gam
    shift = bet - m * scale
    return x * scale + shift, (x - m) * r, m, r


def _gsum32(a, case, order):
    cg = case.cg
    g = a.reshape(a.shape[0], case.groups, cg)
    return np.repeat(osum(lambda c: g[:, :, c], cg, order), cg, 1)


def restate(case, kind, order):
    """What the kernels of this case compute, restated in float32 numpy (no fused multiply-add), sums in `order`."""
    d, fam = inputs(case, kind), case.family
    x = combine32(d["coef"], d["terms"])
    res = {}
    if fam in ("fwd", "pair"):
        xn = gn32(case, x, d["gamma"], d["beta"], d["eps"], order)[0]
        for key, wk in (("S", "W"), ("Sb", "Wb"))[:1 + (fam == "pair")]:
            W = d[wk]
            init = (F32(d["t"]) * W[0])[None, :] if case.has_time else None
            res[key] = matmul32(xn, W[case.has_time:], order, init)
        if case.xout:
            res["xout"] = x
        if case.aux:
            res["aux"] = combine32(d["aux_coef"], d["terms"])
        return res
    if fam in ("bwd", "gn"):
        xn, xh, m, r = gn32(case, x, d["gamma"], d["beta"], d["eps"], order)
        if fam == "gn":
            res["y"], dy = xn, d["dS"]
        else:
            dy = matmul32(d["dS"], np.ascontiguousarray(d["W"][case.has_time:].T), order)
        if case.groups == 0:
            dx = dy
        else:
            cg = case.cg
            gam = np.ones(case.d_in, F32) if d["gamma"] is None else d["gamma"]
            dh = dy * gam
            if bwd_form(case) == "normalised":
                m1 = _gsum32(dh, case, order) * F32(0.25)
                m2 = _gsum32(dh * xh, case, order) * F32(0.25)
                dx = r * (dh - m1 - xh * m2)
            else:
                ds, db = _gsum32(dh * x, case, order), _gsum32(dh, case, order)
                sc = F32(1.0) / F32(cg)
                c2 = (db * m - ds) * (r * r * r * sc)
                c3 = -c2 * m - db * r * sc
                dx = r * gam * dy + c2 * x + c3
            res["dgamma"] = osum(lambda i: dy[i] * xh[i], case.n, order)
            res["dbeta"] = osum(lambda i: dy[i], case.n, order)
        if fam == "bwd":
            dx = F32(d["out_scale"]) * dx
            if case.npre:
                dx = dx + combine32(d["pre_coef"], d["pre"])
        res["dx"] = dx
        return res
    if fam == "wgrad":
        xn = gn32(case, x, d["gamma"], d["beta"], d["eps"], order)[0]
        dS = d["dS"]
        s = osum(lambda i: xn[i][:, None] * dS[i][None, :], case.n, order)
        res["dW"] = np.zeros((case.d_in, case.d_out), F32) if s is None else s
        if case.has_time:
            s0 = osum(lambda i: dS[i], case.n, order)
            res["dW0"] = np.zeros(case.d_out, F32) if s0 is None else s0
        return res
    raise KeyError(fam)


# ---- which case a planted defect changes ------------------------------------------------------------------------------------
def sees_rows(case):
    """Whether a row read or written in the wrong place changes the case's result: not where every row's result is the same."""
    if case.family == "bwd":                                                # dx = 0 at one and two channels per group
        return case.cg == 0 or case.cg >= 3
    return case.cg != 1 or case.xout or case.aux


def sees_terms(case):
    """Whether a dropped or misread term changes the case's result (see the note above SWEEP)."""
    if case.family in ("bwd", "gn"):
        x_matters = case.cg >= 3
    else:
        x_matters = case.cg not in (1, 2) or case.xout or case.aux
    zero = case.kinds == ("exact",) and EXACT_COEF[case.nterms - 1] == 0 and not (case.aux and EXACT_AUX_COEF[case.nterms - 1] != 0)
    return x_matters and not zero


def touches(mut, case):
    """Whether the float64 reference with the defect `mut` differs from the right one on this case (by more than the bound)."""
    fam, cg = case.family, case.cg
    kern = {"fwd": lambda: fwd_kernel(case)[0], "pair": lambda: "pair", "bwd": lambda: bwd_kernel(case)[0],
            "wgrad": lambda: wgrad_kernel(case)[0], "gn": lambda: "gbwd"}[fam]()
    if case.n == 0:
        return False
    if mut == "drop_last_term":
        return case.nterms > 1 and sees_terms(case)
    if mut == "drop_terms_5_8":
        return case.nterms > 4 and sees_terms(case)
    if mut in ("drop_time_row", "time_not_scaled"):
        return bool(case.has_time) and (fam in ("fwd", "pair") or (fam == "wgrad" and mut == "drop_time_row"))
    if mut == "skip_ragged_tile":
        return case.n % _grid(kern, case)[0] != 0
    if mut == "trip2_from_trip1":
        return case.n > first_trip_rows(kern, case) and sees_rows(case)
    if mut == "swap_gamma_beta":
        return bool(case.groups) and not case.gamma_null and fam != "bwd"                   # the VJP is not given beta
    if mut == "w_untransposed":
        return fam == "bwd" and case.d_in == case.d_out and not case.identity
    if mut == "ignore_out_scale":
        return fam == "bwd" and case.out_scale != 1.0 and (cg == 0 or cg >= 3)                # dx = 0 at one and two channels per group
    if mut in ("ignore_pre", "pre_scaled"):
        return fam == "bwd" and case.npre > 0 and (mut == "ignore_pre" or case.out_scale != 1.0)
    if mut == "aux_main_coefs":
        main, aux = (EXACT_COEF, EXACT_AUX_COEF) if case.kinds == ("exact",) else (REAL_COEF, REAL_AUX_COEF)
        return case.aux and main[:case.nterms] != aux[:case.nterms]
    if mut == "pair_sb_with_wa":
        return fam == "pair"
    if mut == "neighbour_group_stats":
        return case.groups > 1 and cg >= 1 and (cg > 1 or fam in ("fwd", "pair", "wgrad", "gn"))
    if mut == "colsum_missing_pass":
        return fam == "wgrad" and kern == "wg" and bool(case.has_time)
    raise KeyError(mut)
