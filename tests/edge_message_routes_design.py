"""Designed inputs and the float64 restatement for the QC edge-message route tests (test_edge_message_routes.py checks the
design's conditions on the CPU, test_gpu_edge_message_routes.py runs the kernels on it).  numpy / CPU torch only; nothing of
the library and nothing of oracle/ is used here.

Eight entry points are covered: gode_edge_matvec_f32_fwd / _msg_f32 / _f32_bwd and gode_edge_outer_sum_f32 (csrc/edge.hip),
gode_edge_ode_feval_f32 / _feval_save_f32 / _vjp_f32 and gode_edge_outer_sum_acc_f32 (csrc/edge_ode.hip).  The limits their
routes branch on are written out below as plain numbers; every case carries the routes it is meant to reach, stated from
those numbers, and test_edge_message_routes.py recomputes them.

A batch is a list of edges (src[e], tgt[e], value[e]); tgt[e] = -1 is an edge without a target.  Its two CSR forms (edges
by target: rowptr / eid, and by source: ms_rowptr / ms_eid) are built here.  `plain` is 12 atoms and 40 edges; `indeg` has
one target of each in-degree 513, 0, 1, 2, 3, 255, 256, 257 at the even atoms (atom 0 and the last atom among them), every odd
atom receiving nothing; `outdeg` has one source of each out-degree 33, 0, 1, 15, 16, 17 the same way; `three` is three edges
on two targets.  Edge ids are shuffled (eid is not the identity) unless the case asks for sorted edges (eid = NULL).

Two kinds of data per case.  `exact`: matrices are integers in -2 .. 2, vectors integers in -4 .. 4, edge values in {1, 2, 3},
coefficients powers of two in 1/4 .. 4 of either sign: every partial sum in ANY order is a multiple of the case's granularity
(1, 1/4 or 1/8) below 2^24 times it (exact_bound: the restatement on the absolute values), so float32 reproduces the float64
result bit for bit and the comparison is torch.equal.  `real`: matrices N(0, 1) / sqrt(h), vectors N(0, 1), edge values
U(0.5, 1.5); compared in the suite's metric max |got - ref| / max(1, max |ref|) at 1e-5 (forward) and 2e-5 (gradients).
The VJP's `fout` is a designed input in both kinds: +0.0, -0.0, negatives and positives.

Conditioning.  test_edge_message_routes.py asserts that a plain float32 restatement stays a factor 4 inside the tolerances
on every case; no case needed another draw (`reseed` is there for one that would).
"""
import functools
import math
import zlib

import numpy as np
import torch

# ---- the limits the routes branch on -------------------------------------------------------------------------------------
MSG_TILE = 8192           # csrc/edge.hip `kMsgTile`: floats of LDS per matrix tile; rpt = max(8192 // h, 1) rows per tile
MSG_XP_MAX_H = 256        # csrc/edge.hip gode_edge_matvec_f32_fwd: edge_matvec_fwd_kernel<1> up to here, <16> above
MSG_HMAX = 4096           # csrc/edge.hip gode_edge_matvec_*: wider -> GODE_E_RANGE
MSG_UNROLL = 8            # csrc/edge.hip lds_dot and the backward's column loop; csrc/edge_ode.hip the VJP's row loop
ROUND = 256               # index triples fetched together: a target with more edges takes another round (both files)
OUTER_HMAX = 1024         # gode_edge_outer_sum_f32 / _acc_f32: wider -> GODE_E_RANGE
MAX_TERMS = 8             # GODE_MAX_TERMS
LDS_DEFAULT = 48 * 1024   # a launch that asks for more dynamic LDS opts in first (gode_set_lds_once)
OUTER_OPTIN = 6144        # 2 n h 4 > 48 KB  <=>  n h > 6144
ODE_HMAX = 112            # csrc/edge_ode.hip `kEdgeOdeMaxH`
ODE_PF = ((32, 4), (64, 16), (112, 49))     # csrc/edge_ode.hip feval_launch: PF by width
FEVAL_UNROLL = 4          # csrc/edge_ode.hip edge_ode_feval_kernel's dot
VJP_ROUND = 16            # csrc/edge_ode.hip `kVjpRound`
THREADS = 256
EDGE_MSG_MIN_EDGES = 256          # ops.py: from here on edge_matvec_fwd is msg + SpMM
EDGE_ODE_FUSED_MAX_EDGES = 4096   # ops.py: from here on the ODE function runs per edge
E_NULLPTR, E_SHAPE, E_RANGE = -1, -2, -4      # include/graphode.h

TOL_FWD, TOL_GRAD = 1e-5, 2e-5    # test_edge_matvec_large_batch_path_matches_fused_path / test_message_chain_forms_the_edge_matrix_gradient_once
PAD = 3                           # strided cases: leading dimension h + 3, base one float past a 16-byte boundary
FORWARD_KEYS = ("out", "msg", "k", "out_save")


# ---- routes, from the numbers above --------------------------------------------------------------------------------------
def msg_tiles(h):
    """(rows per tile, tiles per edge matrix, rows of the last tile)."""
    rpt = max(MSG_TILE // h, 1)
    tiles = -(-h // rpt)
    return rpt, tiles, h - (tiles - 1) * rpt


def matvec_lds(h):
    rpt = msg_tiles(h)[0]
    return (2 * ((h + 3) & ~3) + min(rpt, h) * h) * 4


def feval_lds(h):
    return (h + h * (h + 1)) * 4


def feval_pf(h):
    return next(pf for top, pf in ODE_PF if h <= top)


def vjp_groups(h):
    """(hp, G, rpg, rows of every thread group)."""
    hp = 1
    while hp < h:
        hp <<= 1
    G = THREADS // hp
    rpg = -(-h // G)
    rows = [min(h, min(h, g * rpg) + rpg) - min(h, g * rpg) for g in range(G)]
    return hp, G, rpg, rows


def _round_tags(degrees, per_round, prefix):
    tags = set()
    for d in degrees:
        tags.add("%s%d" % (prefix, min(-(-d // per_round), 3)))
        if d and d % per_round == 0:
            tags.add(prefix + "_full_last")
    return tags


def matvec_route(h, degrees):
    """Tags of edge_matvec_fwd_kernel (and the per-edge kernels' loops) for width h and these in-degrees."""
    rpt, tiles, last = msg_tiles(h)
    tags = {"tiles%s" % (tiles if tiles < 3 else "3+"), "XP1" if h <= MSG_XP_MAX_H else "XP16",
            "lds_optin" if matvec_lds(h) > LDS_DEFAULT else "lds_default", "h%%8==%d" % (h % MSG_UNROLL)}
    if matvec_lds(h) == 64 * 1024:
        tags.add("lds==64K")
    if h < MSG_UNROLL:
        tags.add("tail_only")
    if tiles > 1 and last == 1:
        tags.add("last_tile_one_row")
    if tiles > 1 and 1 < last < rpt:
        tags.add("last_tile_short")
    tags |= _round_tags(degrees, ROUND, "rounds")
    for d in degrees:
        for base in range(0, d, ROUND):
            T = min(ROUND, d - base) * tiles
            tags.add("T==1" if T == 1 else ("T_odd" if T % 2 else "T_even"))
            if tiles > 1:
                tags.add("tiles>1&T_odd" if T % 2 else "tiles>1&T_even")
    return tags


def feval_route(h, degrees):
    tags = {"PF%d" % feval_pf(h), "lds_optin" if feval_lds(h) > LDS_DEFAULT else "lds_default", "h%%4==%d" % (h % FEVAL_UNROLL)}
    if h * h == feval_pf(h) * THREADS:
        tags.add("PF_full")
    return tags | _round_tags(degrees, ROUND, "rounds")


def vjp_route(h, out_degrees):
    hp, G, rpg, rows = vjp_groups(h)
    tags = {"hp%d" % hp, "G%d" % G}
    if any(r >= MSG_UNROLL for r in rows):
        tags.add("unrolled")
    if any(r >= MSG_UNROLL and r % MSG_UNROLL for r in rows):
        tags.add("unrolled_tail")
    if any(0 < r < MSG_UNROLL for r in rows):
        tags.add("tail_only")
    if any(r == 0 for r in rows):
        tags.add("empty_groups")
    if len({r for r in rows if r}) > 1:
        tags.add("short_last_group")
    if hp > h:
        tags.add("idle_columns")
    return tags | _round_tags(out_degrees, VJP_ROUND, "vrounds")


def outer_route(n_terms, h):
    return {"terms%d" % n_terms, "lds_optin" if 2 * n_terms * h * 4 > LDS_DEFAULT else "lds_default"}


# ---- batches ---------------------------------------------------------------------------------------------------------------
IN_DEGREES = (513, 0, 1, 2, 3, 255, 256, 257)
OUT_DEGREES = (33, 0, 1, 15, 16, 17)


class Batch:
    """src / tgt per edge (int32; tgt -1: no target) and the CSR of the edges by target and by source (stable in edge id)."""

    def __init__(self, n, src, tgt):
        self.n, self.E = n, len(src)
        self.src, self.tgt = torch.as_tensor(src, dtype=torch.int32), torch.as_tensor(tgt, dtype=torch.int32)
        self.rowptr, self.eid = self._csr(self.tgt)
        self.ms_rowptr, self.ms_eid = self._csr(self.src)
        self.in_degrees = (self.rowptr[1:] - self.rowptr[:-1]).tolist()
        self.out_degrees = (self.ms_rowptr[1:] - self.ms_rowptr[:-1]).tolist()

    def _csr(self, key):
        key = key.long()
        live = torch.nonzero(key >= 0).flatten()
        order = live[torch.sort(key[live], stable=True)[1]]
        counts = torch.bincount(key[live], minlength=self.n)
        rowptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
        return rowptr.to(torch.int32), order.to(torch.int32)


@functools.lru_cache(maxsize=None)
def batch(kind, sorted_by=None, negrows=False):
    rng = np.random.RandomState({"plain": 11, "indeg": 12, "outdeg": 13, "three": 14}[kind])
    if kind == "plain":
        n = 12
        src, tgt = rng.randint(0, n, 40), rng.randint(0, n - 1, 40)          # the last atom receives nothing
        tgt[:9] = 4                                                          # one target with nine edges
    elif kind == "three":
        n, src, tgt = 3, np.array([1, 2, 0]), np.array([2, 0, 2])
    else:
        degrees = IN_DEGREES if kind == "indeg" else OUT_DEGREES
        n = 2 * len(degrees) - 1
        hub = np.repeat(2 * np.arange(len(degrees)), degrees)
        hub = hub[rng.permutation(len(hub))]
        other = rng.randint(0, n, len(hub))
        src, tgt = (other, hub) if kind == "indeg" else (hub, other)
    if negrows:
        tgt = tgt.copy()
        tgt[[3, len(tgt) - 1]] = -1
    if sorted_by is not None:
        key = np.where(tgt < 0, n, tgt) if sorted_by == "tgt" else src
        order = np.argsort(key, kind="stable")
        src, tgt = src[order], tgt[order]
    return Batch(n, src, tgt)


# ---- case tables ---------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, family, name, h, kind="plain", reaches=(), strided=False, sorted_by=None, noval=False, negrows=False,
                 fwd_only=False, n_terms=0, alpha=1.0, cot_scale=1.0, reseed=0):
        self.family, self.name, self.h, self.kind, self.reaches = family, name, h, kind, set(reaches)
        self.strided, self.sorted_by, self.noval, self.negrows, self.fwd_only = strided, sorted_by, noval, negrows, fwd_only
        self.n_terms, self.alpha, self.cot_scale, self.reseed = n_terms, alpha, cot_scale, reseed

    @property
    def batch(self):
        return batch(self.kind, self.sorted_by, self.negrows)

    def route(self):
        b = self.batch
        if self.family == "matvec":
            return matvec_route(self.h, b.in_degrees)
        if self.family == "feval":
            return feval_route(self.h, b.in_degrees)
        if self.family == "vjp":
            return vjp_route(self.h, b.out_degrees)
        return outer_route(self.n_terms, self.h)

    def __repr__(self):
        return self.name


MATVEC_WIDTHS = (1, 3, 7, 8, 9, 15, 16, 17, 73, 90, 91, 128, 129, 255, 256, 257, 300)
_MATVEC_REACHES = {
    1: {"tail_only", "h%8==1"}, 3: {"tail_only", "h%8==3"}, 7: {"tail_only", "h%8==7"}, 8: {"h%8==0", "tiles1"},
    9: {"h%8==1", "tiles1"}, 15: {"h%8==7"}, 16: {"h%8==0", "tiles1"}, 17: {"h%8==1"}, 73: {"tiles1", "XP1"},
    90: {"tiles1", "h%8==2"}, 91: {"tiles2", "last_tile_one_row", "tiles>1&T_even"}, 128: {"tiles2", "h%8==0"},
    129: {"tiles3+", "last_tile_short", "tiles>1&T_odd", "tiles>1&T_even"}, 255: {"tiles3+", "XP1", "h%8==7"},
    256: {"tiles3+", "XP1"}, 257: {"tiles3+", "XP16", "lds_default"}, 300: {"tiles3+", "XP16", "h%8==4"}}
_DEGREE_REACHES = {"rounds0", "rounds1", "rounds2", "rounds3", "rounds_full_last", "T==1", "T_odd", "T_even"}
MATVEC_CASES = (
    [Case("matvec", "width%d" % h, h, reaches=_MATVEC_REACHES[h]) for h in MATVEC_WIDTHS]
    + [Case("matvec", "rem5_h13", 13, reaches={"h%8==5"}), Case("matvec", "rem6_h14", 14, reaches={"h%8==6"})]   # classes the widths above skip
    + [Case("matvec", "indeg_h16", 16, "indeg", reaches=_DEGREE_REACHES | {"tiles1"}),
       Case("matvec", "indeg_h91", 91, "indeg", reaches={"rounds2", "rounds3", "tiles2", "tiles>1&T_even", "last_tile_one_row"}),
       Case("matvec", "wide2456", 2456, "three", fwd_only=True, reaches={"XP16", "lds_default", "tiles3+"}),
       Case("matvec", "wide2457", 2457, "three", fwd_only=True, reaches={"XP16", "lds_optin", "tiles>1&T_odd"}),
       Case("matvec", "wide4096", 4096, "three", fwd_only=True, reaches={"XP16", "lds_optin", "lds==64K", "tiles>1&T_even"}),
       Case("matvec", "strided_h73", 73, strided=True, reaches={"tiles1", "XP1"}),
       Case("matvec", "strided_h257", 257, strided=True, reaches={"tiles3+", "XP16"}),
       Case("matvec", "eidnull_h16", 16, sorted_by="tgt", reaches={"tiles1"}),
       Case("matvec", "eidnull_h91", 91, sorted_by="tgt", reaches={"tiles2"}),
       Case("matvec", "valnull_h16", 16, noval=True, reaches={"tiles1"}),
       Case("matvec", "valnull_h91", 91, noval=True, reaches={"tiles2"}),
       Case("matvec", "negrow_noval_h9", 9, noval=True, negrows=True, reaches={"h%8==1"}),
       Case("matvec", "negrow_noval_h73", 73, noval=True, negrows=True, reaches={"tiles1"})])

OUTER_CASES = (
    [Case("outer", "terms%d_h73" % n, 73, n_terms=n, reaches={"terms%d" % n, "lds_default"}) for n in (1, 2, 3, 4, 7, 8)]
    + [Case("outer", "terms2_h%d" % h, h, n_terms=2, reaches={"terms2", "lds_default"}) for h in (1, 16, 255, 256, 257)]
    + [Case("outer", "terms8_h768", 768, "three", n_terms=8, reaches={"terms8", "lds_default"}),
       Case("outer", "terms8_h769", 769, "three", n_terms=8, reaches={"terms8", "lds_optin"}),
       Case("outer", "terms8_h1024", 1024, "three", n_terms=8, reaches={"terms8", "lds_optin"}),
       Case("outer", "negrow_noval_t3_h73", 73, n_terms=3, noval=True, negrows=True, reaches={"terms3"}),
       Case("outer", "strided_t3_h73", 73, n_terms=3, strided=True, reaches={"terms3"}),
       Case("outer", "strided_t2_h16", 16, n_terms=2, strided=True, reaches={"terms2"})])

ODE_WIDTHS = (1, 3, 4, 5, 16, 31, 32, 33, 63, 64, 65, 96, 109, 110, 111, 112)
PRE_TERMS, ALPHAS = (0, 1, 3, 8), (1.0, -0.5, 0.25)
COT_TERMS, COT_SCALES = (1, 3, 8), (1.0, -1.0, 0.5)
_FEVAL_REACHES = {
    1: {"PF4", "h%4==1"}, 3: {"PF4", "h%4==3"}, 4: {"PF4", "h%4==0"}, 5: {"PF4", "h%4==1"}, 16: {"PF4"}, 31: {"PF4", "h%4==3"},
    32: {"PF4", "PF_full"}, 33: {"PF16", "h%4==1"}, 63: {"PF16"}, 64: {"PF16", "PF_full"}, 65: {"PF49"}, 96: {"PF49", "lds_default"},
    109: {"PF49", "lds_default"}, 110: {"PF49", "lds_optin", "h%4==2"}, 111: {"PF49", "lds_optin"}, 112: {"PF49", "lds_optin", "PF_full"}}
FEVAL_CASES = (
    [Case("feval", "width%d" % h, h, n_terms=PRE_TERMS[i % 4], alpha=ALPHAS[i % 3], reaches=_FEVAL_REACHES[h])
     for i, h in enumerate(ODE_WIDTHS)]
    + [Case("feval", "indeg_h16", 16, "indeg", n_terms=3, alpha=-0.5, reaches={"rounds0", "rounds1", "rounds2", "rounds3", "rounds_full_last", "PF4"}),
       Case("feval", "indeg_h65", 65, "indeg", n_terms=1, alpha=0.25, reaches={"rounds2", "rounds3", "PF49"}),
       Case("feval", "eidnull_h16", 16, sorted_by="tgt", n_terms=1, reaches={"PF4"}),
       Case("feval", "eidnull_h65", 65, sorted_by="tgt", n_terms=0, alpha=-0.5, reaches={"PF49"}),
       Case("feval", "valnull_h16", 16, noval=True, n_terms=3, alpha=0.25, reaches={"PF4"}),
       Case("feval", "valnull_h65", 65, noval=True, n_terms=8, reaches={"PF49"})])

_VJP_REACHES = {
    1: {"hp1", "G256", "empty_groups"}, 3: {"hp4", "G64", "empty_groups", "idle_columns"}, 4: {"hp4", "G64", "empty_groups"},
    5: {"hp8", "G32", "empty_groups", "idle_columns"}, 16: {"hp16", "G16", "tail_only"}, 31: {"hp32", "G8", "short_last_group"},
    32: {"hp32", "G8", "tail_only"}, 33: {"hp64", "G4", "unrolled_tail", "short_last_group"}, 63: {"hp64", "G4", "unrolled"},
    64: {"hp64", "G4", "unrolled"}, 65: {"hp128", "G2", "unrolled_tail"}, 96: {"hp128", "G2", "unrolled"}, 109: {"hp128", "G2", "unrolled_tail"},
    110: {"hp128", "G2", "unrolled_tail"}, 111: {"hp128", "G2", "unrolled_tail", "short_last_group"}, 112: {"hp128", "G2", "unrolled"}}
_OUT_REACHES = {"vrounds0", "vrounds1", "vrounds2", "vrounds3", "vrounds_full_last"}
VJP_CASES = (
    [Case("vjp", "width%d" % h, h, n_terms=COT_TERMS[i % 3], cot_scale=COT_SCALES[(i // 3) % 3], reaches=_VJP_REACHES[h])
     for i, h in enumerate(ODE_WIDTHS)]
    + [Case("vjp", "outdeg_h%d" % h, h, "outdeg", n_terms=3, cot_scale=0.5, reaches=_OUT_REACHES | r)
       for h, r in ((16, {"tail_only"}), (33, {"unrolled_tail"}), (65, {"unrolled_tail"}), (112, {"unrolled"}))]
    + [Case("vjp", "eidnull_h16", 16, "outdeg", sorted_by="src", n_terms=1, reaches=_OUT_REACHES),
       Case("vjp", "eidnull_h65", 65, sorted_by="src", n_terms=3, cot_scale=-1.0, reaches={"hp128"}),
       Case("vjp", "valnull_h33", 33, noval=True, n_terms=3, reaches={"hp64"}),
       Case("vjp", "negrow_h96", 96, negrows=True, n_terms=1, cot_scale=-1.0, reaches={"hp128"}),
       Case("vjp", "negrow_noval_h5", 5, noval=True, negrows=True, n_terms=8, cot_scale=0.5, reaches={"hp8"})])

ALL_CASES = MATVEC_CASES + OUTER_CASES + FEVAL_CASES + VJP_CASES
BY_NAME = {(c.family, c.name): c for c in ALL_CASES}
PUBLIC_MESSAGE_EDGES = (EDGE_MSG_MIN_EDGES - 1, EDGE_MSG_MIN_EDGES)            # qc_layers.edge_message, h = 9
PUBLIC_FIELD_EDGES = (EDGE_ODE_FUSED_MAX_EDGES - 1, EDGE_ODE_FUSED_MAX_EDGES)  # one EdgeOdeField evaluation and VJP, h = 8


# ---- input builders ------------------------------------------------------------------------------------------------------
COEFS = (1.0, -0.5, 2.0, 0.25, -4.0, 4.0, -0.25, 0.5)             # lincomb coefficients, the first n of them
FOUT_VALUES = (0.0, -0.0, -1.0, 2.0, 0.5, -3.0, 1.0)              # the mask's argument: both zeros, negatives, positives


def outer_weights(n):
    """RK-like weights of the accumulating outer sum: a zero and a negative among them from two terms on."""
    return [-0.5] if n == 1 else list((0.0, -0.5, 2.0, 1.0, -4.0, 0.25, -1.0, 4.0)[:n])


def inputs(case, kind):
    """The case's operands as CPU float32 tensors (lists of tensors for the terms), `kind` = "exact" or "real"."""
    assert kind in ("exact", "real")
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%s/%s" % (case.family, case.name, kind)).encode()) + case.reseed)
    b, h = case.batch, case.h
    if kind == "exact":
        ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()                    # noqa: E731
        mat, vec, ev = (lambda: ints(-2, 2, b.E, h, h)), (lambda *s: ints(-4, 4, *s)), ints(1, 3, b.E)
    else:
        mat = lambda: torch.randn(b.E, h, h, generator=g) / h ** 0.5                                   # noqa: E731
        vec = lambda *s: torch.randn(*s, generator=g)                                                  # noqa: E731
        ev = torch.rand(b.E, generator=g) + 0.5
    d = {"ev": torch.ones(b.E) if case.noval else ev}
    if case.family == "matvec":
        d.update(A=mat(), X=vec(b.n, h), dM=vec(b.n, h))
    elif case.family == "outer":
        d.update(dMs=[vec(b.n, h) for _ in range(case.n_terms)], Xs=[vec(b.n, h) for _ in range(case.n_terms)],
                 w=outer_weights(case.n_terms), dA0=vec(b.E, h, h))
    elif case.family == "feval":
        d.update(A=mat(), X=vec(b.n, h), bias=vec(h), pre=[vec(b.n, h) for _ in range(case.n_terms)], coef=list(COEFS[:case.n_terms]))
    else:
        pick = torch.randint(0, len(FOUT_VALUES), (b.n, h), generator=g)
        pick.view(-1)[:len(FOUT_VALUES)] = torch.arange(len(FOUT_VALUES))          # every value is there at any width
        fout = torch.tensor(FOUT_VALUES)[pick]
        if kind == "real":
            fout = torch.where(fout.abs() > 0, fout * torch.rand(b.n, h, generator=g), fout)
        d.update(A=mat(), cot=[vec(b.n, h) for _ in range(case.n_terms)], coef=list(COEFS[:case.n_terms]), fout=fout)
    return d


def granularity(case):
    """Every intermediate of the case's exact data is a multiple of this."""
    return {"matvec": 1.0, "outer": 0.25, "feval": 0.25, "vjp": 0.125}[case.family]


def strided_block(t):
    """(full, view): t as columns 1 .. 1 + h of a NaN-filled matrix with h + PAD columns."""
    full = torch.full((t.shape[0], t.shape[1] + PAD), float("nan"), dtype=t.dtype)
    full[:, 1:1 + t.shape[1]] = t
    return full, full[:, 1:1 + t.shape[1]]


# ---- the float64 restatement ---------------------------------------------------------------------------------------------
FAULTS = ("drop_edge_257", "drop_last_row_of_last_tile", "skip_last_column", "ignore_edge_value", "gather_at_target", "mask_ge",
          "drop_edge_17", "drop_last_term", "ignore_accumulate")


def _dropped(rowptr, eid, E, position):
    """Edges kept when the one at `position` (0-based) of every CSR row is dropped."""
    keep = torch.ones(E, dtype=torch.bool)
    for v in range(len(rowptr) - 1):
        if rowptr[v + 1] - rowptr[v] > position:
            keep[eid[rowptr[v] + position].long()] = False
    return keep


def _messages(case, d, f, fault):
    """msg[e] = A_e X[src_e] and their per-target sum with the edge values."""
    b, h = case.batch, case.h
    X = f(d["X"])
    ev = torch.ones_like(f(d["ev"])) if fault == "ignore_edge_value" else f(d["ev"])
    src, tgt, live = b.src.long(), b.tgt.long().clamp(min=0), b.tgt >= 0
    xs = X[tgt] if fault == "gather_at_target" else X[src]
    msg = torch.empty(b.E, h, dtype=X.dtype)
    chunk = max(1, (1 << 24) // (h * h))
    for e0 in range(0, b.E, chunk):
        A = f(d["A"][e0:e0 + chunk])
        if fault == "skip_last_column":
            A = A.clone()
            A[:, :, h - 1] = 0
        msg[e0:e0 + chunk] = torch.bmm(A, xs[e0:e0 + chunk].unsqueeze(2)).squeeze(2)
    if fault == "drop_last_row_of_last_tile" and msg_tiles(h)[1] > 1:
        msg[:, h - 1] = 0
    if fault == "drop_edge_257":
        live = live & _dropped(b.rowptr, b.eid, b.E, ROUND)
    total = torch.zeros(b.n, h, dtype=X.dtype).index_add(0, tgt[live], (ev[:, None] * msg)[live])
    return msg, total


def _caster(dtype, absolute):
    return lambda t: (t.abs() if absolute else t).to(dtype)


def matvec_reference(case, d, dtype=torch.float64, fault=None, absolute=False):
    """out / msg of the forward entry points, dA / dxe of the backward."""
    f = _caster(dtype, absolute)
    b = case.batch
    msg, out = _messages(case, d, f, fault)
    res = {"out": out, "msg": msg}
    if not case.fwd_only:
        A, X, dM = f(d["A"]), f(d["X"]), f(d["dM"])
        ev = torch.ones_like(f(d["ev"])) if fault == "ignore_edge_value" else f(d["ev"])
        dm = ev[:, None] * dM[b.tgt.long().clamp(min=0)] * (b.tgt >= 0).to(dtype)[:, None]
        res["dA"] = dm[:, :, None] * X[b.src.long()][:, None, :]
        res["dxe"] = torch.bmm(A.transpose(1, 2), dm.unsqueeze(2)).squeeze(2)
    return res


def feval_reference(case, d, dtype=torch.float64, fault=None, absolute=False):
    """k = relu(sum + bias), out = (sum pre) + alpha k."""
    f = _caster(dtype, absolute)
    z = _messages(case, d, f, fault)[1] + f(d["bias"])
    k = z if absolute else torch.relu(z)
    out = (abs(case.alpha) if absolute else case.alpha) * k
    for c, t in zip(d["coef"], d["pre"]):
        out = out + (abs(c) if absolute else c) * f(t)
    return {"out": out, "k": k}


def vjp_reference(case, d, dtype=torch.float64, fault=None, absolute=False):
    """dM = cot_scale (sum cot) [fout > 0], dxe[e] = A_e^T (val_e dM[tgt_e]), dS = its sum per source."""
    f = _caster(dtype, absolute)
    b, h = case.batch, case.h
    g = torch.zeros(b.n, h, dtype=dtype)
    for c, t in zip(d["coef"], d["cot"]):
        g = g + (abs(c) if absolute else c) * f(t)
    g = (abs(case.cot_scale) if absolute else case.cot_scale) * g
    if not absolute:
        open_ = d["fout"] >= 0 if fault == "mask_ge" else d["fout"] > 0
        g = torch.where(open_, g, torch.zeros_like(g))
    ev = torch.ones_like(f(d["ev"])) if fault == "ignore_edge_value" else f(d["ev"])
    live = b.tgt >= 0
    dm = ev[:, None] * g[b.tgt.long().clamp(min=0)] * live.to(dtype)[:, None]
    dxe = torch.bmm(f(d["A"]).transpose(1, 2), dm.unsqueeze(2)).squeeze(2)
    keep = _dropped(b.ms_rowptr, b.ms_eid, b.E, VJP_ROUND) if fault == "drop_edge_17" else torch.ones(b.E, dtype=torch.bool)
    dS = torch.zeros(b.n, h, dtype=dtype).index_add(0, b.src.long()[keep], dxe[keep])
    return {"dM": g, "dS": dS, "dxe": dxe}


def outer_reference(case, d, dtype=torch.float64, fault=None, absolute=False):
    """plain = sum_t (val dM_t[tgt]) (x) X_t[src]; over = the same with the weights; acc = dA0 + over."""
    f = _caster(dtype, absolute)
    b = case.batch
    ev = torch.ones_like(f(d["ev"])) if fault == "ignore_edge_value" else f(d["ev"])
    gate = ev * (b.tgt >= 0).to(dtype)
    tgt, src = b.tgt.long().clamp(min=0), b.src.long()
    n = case.n_terms - 1 if fault == "drop_last_term" else case.n_terms
    plain = torch.zeros(b.E, case.h, case.h, dtype=dtype)
    over = torch.zeros_like(plain)
    for t in range(n):
        term = (gate[:, None] * f(d["dMs"][t])[tgt])[:, :, None] * f(d["Xs"][t])[src][:, None, :]
        plain = plain + term
        over = over + (abs(d["w"][t]) if absolute else d["w"][t]) * term
    return {"plain": plain, "over": over, "acc": over if fault == "ignore_accumulate" else f(d["dA0"]) + over}


REFERENCES = {"matvec": matvec_reference, "feval": feval_reference, "vjp": vjp_reference, "outer": outer_reference}


def reference(case, d, dtype=torch.float64, fault=None, absolute=False):
    return REFERENCES[case.family](case, d, dtype, fault, absolute)


def exact_bound(case, d):
    """The largest sum of absolute values behind any result of the exact data, in units of the granularity: below 2^24
    every partial sum in every order is a float32 number."""
    return max(t.max().item() for t in reference(case, d, absolute=True).values()) / granularity(case)


# ---- comparison ----------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """The suite's `close` metric: max |got - ref| / max(1, max |ref|); inf for a wrong shape or a NaN."""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    if got.shape != ref.shape:
        return math.inf
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs().max().item()
    return math.inf if math.isnan(err) else err / max(1.0, ref.abs().max().item())


def tolerance(key):
    return TOL_FWD if key in FORWARD_KEYS else TOL_GRAD


def errors(got, ref):
    return {k: rel_err(got[k], ref[k]) for k in ref if k in got}


def failures(errs):
    return [k for k, e in errs.items() if not e <= tolerance(k)]


def unequal(got, ref):
    """Keys whose result is not the float64 one rounded to float32 (exact data)."""
    return [k for k in ref if k in got and not (got[k].shape == ref[k].shape and torch.equal(got[k].detach().cpu().float(), ref[k].float()))]
