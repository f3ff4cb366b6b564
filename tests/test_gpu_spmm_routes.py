"""Every SpMM route, record shape and epilogue of csrc/spmm.hip against an exact reference.

Exact data.  Matrix values are integers in 1..3 (or pattern-only), X / bias / pre / cot are integers in -8..8 and every
coefficient and alpha is a power of two in 1/4..4 of either sign.  The longest row has 1 000 entries, so
|z| <= 1000 * 3 * 8 + 8 = 24 008 and every intermediate of Y = sum pre + alpha * act(Z) is a multiple of 1/4 below
4 * 24 008 + 8 * 4 * 8 < 2^17: all of them are fp32 numbers, the result does not depend on the order of the sums, and
the comparison with the float64 CPU reference (torch.sparse.mm and dense ops, following the docstring of ops.spmm) is
BIT FOR BIT.  Integer data makes Z == 0 frequent, so `>` against `>=` in the cotangent mask is really tested.

Designed graphs (design()): 66 003 rows (more than 65 536 records) and 1 500 rows, m = 4099 columns, split = 96, their
twins without a record list, their transposes, and two sizes with exactly 65 536 and 65 537 records.  Rows of every record length the inner loops branch on
(SHORT: each lane-group width d/4 in 1..64 and its neighbours, the wave kernel's stride of 64, every remainder of the
4-way unroll, 95 / 96 at the split length) and split rows (LONG: 2, 3, 4, 5, 9 and 11 slots - the finishing kernel's
4-way unrolled loop runs 0, 1 and 2 times with tails of 0, 1, 2 and 3) sit at chosen rows, row 0 and the last row
included, each beside an empty row; the rest are rows of 1..3 entries.  A few rows repeat a column, columns 0 and m - 1
occur, and one hub column makes the transpose have split rows too.  (The degree of 384 is there for the 4 slots that
leave the unrolled loop without a tail.)

Routes.  Each launch runs under the library's launch profile, which brackets the 16-byte-lane kernels and the one-column
kernel (recording the width) and not the generic kernel; with ops.spmm_y2_colsum_rows (> 0: a thread group per record,
0: a wave per record / generic) that tells the four main kernels apart, so no case can silently test another kernel.
"""
import contextlib
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

M = 4099
SPLIT = 96
SHORT = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96]
LONG = [97, 192, 193, 288, 384, 389, 480, 769, 863, 1000]
SLOT_COUNTS = {2, 3, 4, 5, 9, 11}
EXTRA = sum(-(-deg // SPLIT) - 1 for deg in LONG)         # records beyond one per row
HUB_COL = 7
N_OF = {"L": 66_003, "S": 1_500, "B0": 65_536 - EXTRA, "B1": 65_537 - EXTRA}     # B0 / B1: n_items == 65 536 / 65 537
VEC4 = [4, 8, 16, 32, 64, 128, 256]
GENERIC = [1, 7, 12, 20, 73, 260, 512]
SENTINEL = 77.0


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# the designed graphs (numpy / CPU torch only: the unmarked test below runs all of this without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
def base_of(kind):
    return kind[:2] if kind[0] == "B" else kind[0]


@functools.lru_cache(maxsize=None)
def design(n):
    """(rowptr, col, val, {row: degree} of the special rows, rows with a repeated column) of the n x M designed matrix;
    val are integers 1..3."""
    rs = np.random.RandomState(n)
    special = [1000] + SHORT + [x for x in LONG if x not in (1000, 863)] + [863]
    pos = np.round(np.linspace(0, n - 1, len(special))).astype(np.int64)
    assert len(set(pos.tolist())) == len(special) and pos[0] == 0 and pos[-1] == n - 1
    deg = rs.randint(1, 4, n)
    is_bulk = np.ones(n, bool)
    for p, s in zip(pos, special):
        e = p + 1 if p + 1 < n else p - 1              # an empty row beside every special row
        deg[p], deg[e] = s, 0
        is_bulk[p] = is_bulk[e] = False
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    nnz = int(rowptr[-1])
    col = rs.randint(0, M, nnz)
    val = rs.randint(1, 4, nnz).astype(np.float32)
    hub = is_bulk & (rs.randint(0, 8, n) == 0)          # one column in 1/8 of the bulk rows: a split row of the transpose
    col[rowptr[:-1][hub]] = HUB_COL
    col[0], col[2], col[nnz - 1], col[rowptr[n - 1]] = 0, M - 1, M - 1, 0
    rep = [int(p) for p, s in zip(pos, special) if s in (5, 17, 97, 1000)]
    rep += [int(r) for r in np.nonzero(is_bulk & (deg >= 2))[0][:3]]
    for r in rep:                                       # a repeated column: the entries of a row are a multiset
        col[rowptr[r] + 1] = col[rowptr[r]]
    return rowptr, col, val, dict(zip(pos.tolist(), special)), tuple(rep)


def float_values(n):
    """Values in [0.1, 1.1) on the designed pattern (the rounding cases)."""
    nnz = int(design(n)[0][-1])
    return (np.random.RandomState(n + 1).rand(nnz) * 1.0 + 0.1).astype(np.float32)


def make_graph(kind, values, device):
    """kind: L / S / B0 / B1, + 'nr' (no record list) or 'T' (transpose); values: 'int', 'pattern' or 'float'."""
    from graph_odenet_amd import graph as G
    n = N_OF[base_of(kind)]
    rowptr, col, val, _, _ = design(n)
    v = {"int": val, "pattern": None, "float": float_values(n) if values == "float" else None}[values]
    g = G.CSRGraph(torch.from_numpy(rowptr).to(device), torch.from_numpy(col).to(device),
                   None if v is None else torch.from_numpy(v).to(device), n, M, split=SPLIT, records=not kind.endswith("nr"))
    return g.transpose() if kind.endswith("T") else g


@functools.lru_cache(maxsize=None)
def ref_matrix(kind, values, absolute=False):
    """The same matrix as a float64 CPU sparse tensor, built from design() alone (duplicates summed by coalesce)."""
    n = N_OF[base_of(kind)]
    rowptr, col, val, _, _ = design(n)
    v = {"int": val, "pattern": np.ones(col.size, np.float32), "float": float_values(n) if values == "float" else None}[values]
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    idx = torch.from_numpy(np.stack([rows, col]))
    v = torch.from_numpy(v).double()
    A = torch.sparse_coo_tensor(idx, v.abs() if absolute else v, (n, M))
    if kind.endswith("T"):
        A = A.t()
    return A.coalesce()


def shape_of(kind):
    n = N_OF[base_of(kind)]
    return (M, n) if kind.endswith("T") else (n, M)


def ints(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=gen, dtype=torch.float32)


@functools.lru_cache(maxsize=4)
def x_ints(rows, d):
    return ints((rows, d), 1000 + d)


@functools.lru_cache(maxsize=2)
def z_ref(kind, values, d):
    """A @ X in float64 on the CPU (kind without 'nr': the record list does not change the product)."""
    return torch.sparse.mm(ref_matrix(kind, values), x_ints(shape_of(kind)[1], d).double())


def z_of(kind, values, d):
    return z_ref(kind[:-2] if kind.endswith("nr") else kind, values, d)


def pow2(rs):
    return float(2.0 ** rs.randint(-2, 3) * (1 if rs.randint(0, 2) else -1))


def reference(Z, bias=None, relu=False, alpha=1.0, pre=(), cot=(), c3=None):
    """The documented formula of ops.spmm in float64: Y, Y2, Y3, K."""
    Zb = Z if bias is None else Z + bias.double()
    K = Zb.clamp_min(0) if relu else Zb
    Y = alpha * K
    for c, p in pre:
        Y = Y + c * p.double()
    Y2 = Y3 = None
    if cot:
        Y2 = sum(c * t.double() for c, t in cot) * (Zb > 0)           # the mask holds whether or not relu is set
        if c3 is not None:
            Y3 = sum(c * t.double() for c, (_, t) in zip(c3, cot))
    return Y, Y2, Y3, K


# ---------------------------------------------------------------------------------------------------------------------
# rounding cases: inputs and the derived bound, from the float64 reference alone
# ---------------------------------------------------------------------------------------------------------------------
ROUNDING = [("L", 128, "tg"), ("S", 32, "wave"), ("S", 256, "tg"), ("L", 73, "generic"), ("S", 20, "generic"), ("S", 1, "spmv")]
F32 = lambda x: float(np.float32(x))
PRE_C = [F32(0.3), F32(-0.7), F32(1.1), F32(0.45)]
COT_C = [F32(-1.3), F32(0.6), F32(0.9), F32(-0.35)]
COT3_C = [F32(0.15), F32(1.7), F32(-0.55), F32(0.8)]
ALPHA_R = F32(-0.37)
U2 = 2.0 ** -23


@functools.lru_cache(maxsize=1)
def rounding_problem(kind, d):
    """X ~ N(0, 1), values in [0.1, 1.1), bias ~ N(0, 1); Z64 = A X + b of the fp32 inputs in float64, and per element

        |Z - Z64|_ij <= 2^-23 * (deg_i + nseg_i + 3) * (sum_k |a_ik| |x_kj| + |b_j|).

    Derivation.  Whatever the order in which a kernel adds the deg_i products of a row (a chain per lane group, 64 / LPR
    chains joined by xor-shuffles, 64 strided chains joined by a wave sum, partial sums of <= 96 entries joined by the
    finishing kernel), a product passes through its own fused multiply-add, at most deg_i - 1 additions with a
    non-zero partner (adding zero is exact), at most nseg_i additions of partial sums and the addition of the bias:
    at most k = deg_i + nseg_i + 1 roundings of relative size u = 2^-24.  The error is then at most
    ((1 + u)^k - 1) * sum |terms| <= 2 k u * sum |terms| for k u < 1 (k <= 1 014 here); the factor 2 over u is in 2^-23."""
    assert kind in ("L", "S")
    n_rows, n_cols = shape_of(kind)
    gen = torch.Generator().manual_seed(77 + d)
    X = torch.randn(n_cols, d, generator=gen)
    b = torch.randn(d, generator=gen)
    Z = torch.sparse.mm(ref_matrix(kind, "float"), X.double()) + b.double()
    mag = torch.sparse.mm(ref_matrix(kind, "float", True), X.double().abs()) + b.double().abs()
    deg = torch.from_numpy(np.diff(design(N_OF[base_of(kind)])[0])).double()
    nseg = torch.clamp(torch.ceil(deg / SPLIT), min=1)
    bound = U2 * (deg + nseg + 3)[:, None] * mag
    return X, b, Z, bound


def kink_share(kind, d):
    _, _, Z, bound = rounding_problem(kind, d)
    return float((Z.abs() <= bound).double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# the one CPU test: everything the GPU tests rely on
# ---------------------------------------------------------------------------------------------------------------------
def test_designed_graphs_have_the_records_the_cases_rely_on():
    cpu = torch.device("cpu")
    for kind in ("L", "S", "B0", "B1"):
        n = N_OF[kind]
        rowptr, col, val, special, rep = design(n)
        g = make_graph(kind, "int", cpu)
        assert g.n_items == n + EXTRA and g.n_long == len(LONG) and g.n_slots == EXTRA + len(LONG)
        lens = set((g.items[:, 2] - g.items[:, 1]).tolist())
        assert set(SHORT) <= lens and max(lens) == SPLIT, sorted(lens)
        assert set((x % SPLIT) for x in LONG if x % SPLIT) <= lens             # the last records of the split rows
        slots = (g.long_rows[:, 2] - g.long_rows[:, 1]).tolist()
        assert set(slots) == SLOT_COUNTS and {s % 4 for s in slots} == {0, 1, 2, 3}, slots
        deg = np.diff(rowptr)
        assert special[0] == 1000 and special[n - 1] == 863                    # split rows first and last
        for p, s in special.items():
            assert deg[p] == s and deg[p + 1 if p + 1 < n else p - 1] == 0
        assert col.min() == 0 and col.max() == M - 1 and col[0] == 0 and col[-1] == M - 1
        for r in rep:
            assert col[rowptr[r]] == col[rowptr[r] + 1]
        assert ref_matrix(kind, "int")._nnz() < col.size                       # repeated columns are summed there
        # exactness: |z| <= 24 008, and 4 * (4 |z| + 8 terms * 4 * 8) far below 2^24
        zmax = float(torch.from_numpy(np.add.reduceat(val, rowptr[:-1][deg > 0])).max()) * 8 + 8
        assert zmax <= 24_008 and 4 * (4 * zmax + 8 * 4 * 8) < 2 ** 22
        # the record-less twin walks whole rows
        gn = make_graph(kind + "nr", "int", cpu)
        assert gn.items is None and gn.n_items == n and gn.n_long == 0 and gn.partial(16) is None
        # the transpose has split rows of its own (the hub column) and rows of many lengths
        gt = make_graph(kind + "T", "int", cpu)
        assert gt.n_rows == M and gt.n_cols == n and gt.n_long >= 1 and gt.n_items <= 65_536
        assert HUB_COL in gt.long_rows[:, 0].tolist()
        if kind == "S":
            assert torch.equal(gt.to_dense().double(), ref_matrix("ST", "int").to_dense())
            assert torch.equal(g.to_dense().double(), ref_matrix("S", "int").to_dense())
    assert make_graph("L", "int", cpu).n_items > 65_536
    assert make_graph("B0", "int", cpu).n_items == 65_536 and make_graph("B1", "int", cpu).n_items == 65_537
    assert make_graph("S", "int", cpu).n_items == 1_500 + EXTRA
    # a partly filled last block in the main and in the finishing launch
    for kind, ds in (("L", (16, 128, 256)), ("B1", (16, 128)), ("S", (256,)), ("Lnr", (16, 128, 256))):
        g = make_graph(kind, "pattern", cpu)
        for d in ds:
            assert (g.n_items * (d // 4)) % 256 != 0, (kind, d)
            assert kind.endswith("nr") or (g.n_long * (d // 4)) % 256 != 0, (kind, d)
    # the share of entries within rounding of the relu kink, from the reference alone
    for kind, d, _ in ROUNDING:
        share = kink_share(kind, d)
        print("kink share %s d=%d: %.2e" % (kind, d, share))
        assert share <= 1e-4, (kind, d, share)


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
_graphs = {}


def gpu_graph(kind, values):
    key = (kind, values)
    if key not in _graphs:
        _graphs[key] = make_graph(kind, values, dev())
    return _graphs[key]


@contextlib.contextmanager
def profile():
    """Widths recorded by the profiled launches of the body (the 16-byte-lane kernels and the one-column kernel)."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    prof = lib.gode_prof_create(8)
    assert prof
    out = []
    lib.gode_prof_enable(prof)
    try:
        yield out
        torch.cuda.synchronize()
        n = lib.gode_prof_count(prof)
        if n:
            ms, dd = (ctypes.c_float * n)(), (ctypes.c_int64 * n)()
            assert lib.gode_prof_read(prof, ms, dd, None, None, n) == n
            out.extend(int(x) for x in dd)
    finally:
        lib.gode_prof_enable(None)
        lib.gode_prof_destroy(prof)


def natural_route(kind, d):
    """The route a launch with aligned operands takes, by the design of the graphs."""
    if d == 1:
        return "generic" if kind.endswith("nr") else "spmv"
    if d not in VEC4:
        return "generic"
    big = kind in ("L", "Lnr", "B1")
    return "tg" if (big or d == 256) else "wave"


def assert_route(route, g, d, widths, forced=False):
    from graph_odenet_amd import ops
    rows = ops.spmm_y2_colsum_rows(g, d)
    if route == "tg":
        assert rows > 0 and widths == [d], (rows, widths)
    elif route == "wave":
        assert rows == 0 and widths == [d] and d > 1, (rows, widths)
    elif route == "spmv":
        assert rows == 0 and widths == [1] and d == 1 and g.items is not None, (rows, widths)
    else:
        assert widths == [] and (forced or rows == 0), (rows, widths)


def same(got, want, what):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, bad.shape[0], want.numel(), i, got[i].item(), want[i].item()))


def offset_copy(t):
    """A contiguous copy of t whose pointer misses 16-byte alignment by one element."""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev())
    flat[1:].copy_(t.reshape(-1))
    out = flat[1:].view(t.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def colsum_partial_reference(g, d, Y2):
    """Per-block column sums of Y2 from the documented layout: block b of the main launch holds the records
    [b * 256 / LPR, (b + 1) * 256 / LPR), of which those with slot < 0 store a row; the finishing launch's rows follow."""
    per = 256 // (d // 4)
    if g.items is not None:
        items = g.items.cpu().long()
        rec = torch.nonzero(items[:, 3] < 0).flatten()
        rows = items[rec, 0]
    else:
        rec = torch.arange(g.n_rows)
        rows = rec
    nb = (g.n_items * (d // 4) + 255) // 256
    nb2 = (g.n_long * (d // 4) + 255) // 256
    want = torch.zeros(nb + nb2, d, dtype=torch.float64)
    want.index_add_(0, rec // per, Y2[rows])
    if g.n_long:
        lr = g.long_rows.cpu().long()
        want.index_add_(0, nb + torch.arange(g.n_long) // per, Y2[lr[:, 0]])
    return want


def spmm_save(g, X, out, K, bias, relu, alpha, pre_terms):
    """gode_spmm_csr_save_f32: ops.spmm's launch, which also stores K = act(Z + bias) with ld = d."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    d = X.shape[1]
    ep = _lib.SpmmEpilogue()
    ep.bias = bias.data_ptr() if bias is not None else None
    ep.relu = 1 if relu else 0
    ep.alpha = float(alpha)
    if pre_terms:
        ep.pre = _lib.lincomb(pre_terms)
    assert out.stride(1) == 1 and K.is_contiguous() and tuple(K.shape) == (g.n_rows, d)
    rc = lib.gode_spmm_csr_save_f32(_lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val), _lib.ptr(g.items), g.n_items,
                                    _lib.ptr(g.long_rows), g.n_long, _lib.ptr(g.partial(d)), _lib.ptr(X), d,
                                    _lib.ptr(out), out.stride(0), g.n_rows, d, ctypes.byref(ep), _lib.ptr(K),
                                    _lib.stream_ptr())
    _lib.check(rc, "gode_spmm_csr_save_f32")


def run_exact(kind, values, d, route, seed, bias=False, relu=False, alpha=1.0, n_pre=0, n_cot=0, third=False, alias=False,
              save=False, colsum=False, layout="plain", forced=False):
    """One launch on exact data against the float64 reference, bit for bit, with its route asserted."""
    from graph_odenet_amd import ops
    g = gpu_graph(kind, values)
    n = g.n_rows
    X = x_ints(g.n_cols, d)
    Z = z_of(kind, values, d)
    rs = np.random.RandomState(seed)
    b = ints((d,), seed + 1) if bias else None
    pre = [(1.0 if alias else pow2(rs), ints((n, d), seed + 10 + j)) for j in range(n_pre)]
    cot = [(pow2(rs), ints((n, d), seed + 30 + j)) for j in range(n_cot)]
    c3 = [pow2(rs) for _ in cot] if third else None
    Yr, Y2r, Y3r, Kr = reference(Z, b, relu, alpha, pre, cot, c3)

    Xd = offset_copy(X) if layout == "x_off" else X.to(dev())
    bd = None if b is None else (offset_copy(b) if layout == "bias_off" else b.to(dev()))
    pre_d = [(c, offset_copy(t) if (layout == "pre_off" and j == 0) else t.to(dev())) for j, (c, t) in enumerate(pre)]
    cot_d = [(c, offset_copy(t) if (layout == "cot_off" and j == len(cot) - 1) else t.to(dev())) for j, (c, t) in enumerate(cot)]
    buf, out = None, None
    if layout == "wide":                                   # aligned for the 16-byte-lane widths, ldy != d
        buf = torch.full((n, 2 * d + 4), SENTINEL, device=dev())
        out, lo = buf[:, :d], 0
    elif layout == "off2":                                 # two columns into a wider matrix: the pointer misses alignment
        buf = torch.full((n, d + 4), SENTINEL, device=dev())
        out, lo = buf[:, 2:2 + d], 2
    elif layout == "ld_odd":                               # ldy % 4 != 0
        buf = torch.full((n, d + 1), SENTINEL, device=dev())
        out, lo = buf[:, :d], 0
    elif alias:
        out = pre_d[0][1]                                  # the drivers' in-place close: Y = 1.0 * Y + alpha * K
    kw = {}
    part = None
    if colsum:
        part = torch.full((ops.spmm_y2_colsum_rows(g, d), d), float("nan"), device=dev())
        kw["out2_colsum"] = part
    Y3 = None
    if third:
        Y3 = torch.full((n, d), float("nan"), device=dev())
        kw.update(cot_out=Y3, cot_out_coefs=c3)
    K = None
    with profile() as widths:
        if save:
            K = torch.full((n, d), float("nan"), device=dev())
            if out is None:
                out = torch.empty(n, d, device=dev())
            spmm_save(g, Xd, out, K, bd, relu, alpha, pre_d)
            res = out
        else:
            res = ops.spmm(g, Xd, bias=bd, relu=relu, out=out, alpha=alpha, pre_terms=pre_d or None, cot_terms=cot_d or None, **kw)
    assert_route(route, g, d, widths, forced)
    Y, Y2 = res if cot else (res, None)
    what = "%s %s d=%d %s" % (kind, values, d, layout)
    same(Y, Yr, what + ": Y")
    if buf is not None:
        keep = torch.ones(buf.shape[1], dtype=torch.bool, device=dev())
        keep[lo:lo + d] = False
        assert bool((buf[:, keep] == SENTINEL).all()), what + ": a neighbouring column was written"
    if cot:
        same(Y2, Y2r, what + ": Y2")
    if third:
        same(Y3, Y3r, what + ": Y3")
    if save:
        same(K, Kr, what + ": K")
    if colsum:
        assert part.shape[0] > 0
        same(part, colsum_partial_reference(g, d, Y2r), what + ": per-block column sums")
        assert torch.equal(part.double().sum(0).cpu(), Y2r.sum(0)), what + ": column-sum total"
        assert torch.equal(part.double().sum(0), Y2.double().sum(0))


# -- every width, weighted and pattern-only, on both graphs, their record-less twins and their transposes -------------
WIDTH_CASES = [(kind, d, values) for d in VEC4 + GENERIC for values in ("int", "pattern")
               for kind in ("L", "Lnr", "S", "Snr", "LT", "ST")]


@gpu
@pytest.mark.parametrize("kind,d,values", WIDTH_CASES, ids=["%s-%d-%s" % c for c in WIDTH_CASES])
def test_every_width_exact(kind, d, values):
    """The plain product, then bias + relu + alpha + 2 pre + 2 cot + the third output in one launch (with the per-block
    column sums where the route forms them), on every width of both routes' tables."""
    route = natural_route(kind, d)
    run_exact(kind, values, d, route, seed=d)
    run_exact(kind, values, d, route, seed=d + 1, bias=True, relu=True, alpha=-0.5, n_pre=2, n_cot=2, third=True,
              colsum=route == "tg")


# -- every epilogue on every route ----------------------------------------------------------------------------------
EPILOGUES = {
    "plain": dict(),
    "bias": dict(bias=True),
    "bias_relu": dict(bias=True, relu=True),
    "alpha": dict(alpha=-0.25),
    "alpha_relu": dict(alpha=4.0, relu=True, bias=True),
    "pre1": dict(n_pre=1, alpha=2.0),
    "pre8": dict(n_pre=8, alpha=-0.5, bias=True, relu=True),
    "cot1": dict(n_cot=1),
    "cot8": dict(n_cot=8, bias=True),
    "cot1_relu": dict(n_cot=1, relu=True, bias=True),
    "cot8_relu": dict(n_cot=8, relu=True),
    "cot_out": dict(n_cot=4, third=True, bias=True, relu=True),
    "cot_out8": dict(n_cot=8, third=True, n_pre=8, alpha=0.5),
    "alias": dict(n_pre=1, alias=True, alpha=0.25, bias=True, relu=True),
    "save": dict(save=True, bias=True, relu=True, n_pre=2, alpha=-2.0, layout="wide"),
    "save_plain": dict(save=True),
}
ROUTE_REPS = [("L", 128, "int"), ("L", 16, "pattern"), ("Lnr", 128, "int"), ("S", 256, "int"),            # thread group
              ("S", 32, "int"), ("S", 4, "pattern"), ("Snr", 16, "int"), ("LT", 64, "int"),                # wave
              ("L", 12, "int"), ("S", 73, "pattern"), ("Lnr", 20, "int"), ("Snr", 1, "int"), ("ST", 260, "int"),   # generic
              ("L", 1, "int"), ("S", 1, "pattern"), ("LT", 1, "int")]                                      # one column
EPILOGUE_CASES = [(k, d, v, e) for (k, d, v) in ROUTE_REPS for e in EPILOGUES]


@gpu
@pytest.mark.parametrize("kind,d,values,epilogue", EPILOGUE_CASES, ids=["%s-%d-%s-%s" % c for c in EPILOGUE_CASES])
def test_every_epilogue_exact(kind, d, values, epilogue):
    """Split rows go through the same epilogue in the finishing kernels: every graph here has them (the record-less
    twins walk them whole)."""
    route = natural_route(kind, d)
    kw = dict(EPILOGUES[epilogue])
    if route == "tg" and kw.get("n_cot"):
        kw["colsum"] = True
    run_exact(kind, values, d, route, seed=500 + len(epilogue) + d, **kw)


# -- alignment: the 16-byte-lane widths pushed onto the generic kernels, and kept off it with ldy != d ---------------
ALIGN_CASES = [(k, d, lay) for (k, d) in (("L", 128), ("L", 16), ("S", 64), ("S", 256), ("Snr", 8), ("ST", 32))
               for lay in ("wide", "off2", "ld_odd", "bias_off", "x_off", "pre_off", "cot_off")]


@gpu
@pytest.mark.parametrize("kind,d,layout", ALIGN_CASES, ids=["%s-%d-%s" % c for c in ALIGN_CASES])
def test_alignment_decides_the_route(kind, d, layout):
    """`wide` (ldy = 2 d + 4) stays on the 16-byte-lane kernels and leaves the neighbouring columns alone; an output two
    columns into a wider matrix, ldy % 4 != 0, and a bias / X / pre / cot operand whose pointer alone misses 16 bytes
    all run the generic kernels (where a request for per-block column sums is refused)."""
    from graph_odenet_amd import ops
    full = dict(bias=True, relu=True, alpha=2.0, n_pre=2, n_cot=2, third=True)
    if layout == "wide":
        run_exact(kind, "int", d, natural_route(kind, d), seed=900 + d, layout=layout, **full)
        return
    run_exact(kind, "int", d, "generic", seed=900 + d, layout=layout, forced=True, **full)
    g = gpu_graph(kind, "int")
    if layout == "x_off" and ops.spmm_y2_colsum_rows(g, d) > 0:
        Xd = offset_copy(x_ints(g.n_cols, d))
        t = torch.zeros(g.n_rows, d, device=dev())
        with pytest.raises(RuntimeError):
            ops.spmm(g, Xd, relu=True, cot_terms=[(1.0, t)],
                     out2_colsum=torch.empty(ops.spmm_y2_colsum_rows(g, d), d, device=dev()))


# -- the dispatch boundary ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("kind", ["B0", "B1"])
def test_dispatch_boundary(kind, d):
    """65 536 records run a wave per record, 65 537 a thread group per record; both equal the reference."""
    g = gpu_graph(kind, "int")
    assert g.n_items == (65_536 if kind == "B0" else 65_537)
    route = "wave" if kind == "B0" else "tg"
    run_exact(kind, "int", d, route, seed=40 + d, bias=True, relu=True, alpha=-0.5, n_pre=1, n_cot=2, colsum=route == "tg")


# -- operand arrays beyond 2^32 bytes ---------------------------------------------------------------------------------
@gpu
def test_operands_beyond_4_gib():
    """n = m = 2^23 + 3 rows of d = 128: X, Y, Y2 and the pre-term each hold more than 2^32 bytes, the smallest shape at
    which a 32-bit byte offset wraps.  One entry per row (the first rows gather the last rows of X and the other way
    round), the last row a split row of 200 entries.  Inputs and reference are formed on the GPU from the same integers."""
    from graph_odenet_amd import graph as G, ops
    t0 = time.time()
    n, d, hub = 2 ** 23 + 3, 128, 200
    gen = torch.Generator(device=dev()).manual_seed(3)
    deg = torch.ones(n, dtype=torch.int64, device=dev())
    deg[n - 1] = hub
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev())
    rowptr[1:] = torch.cumsum(deg, 0)
    nnz = n - 1 + hub
    col = torch.randint(0, n, (nnz,), generator=gen, device=dev())
    col[:64] = n - 1 - torch.arange(64, device=dev())                 # the highest rows of X
    col[n - 2], col[nnz - 1] = 0, n - 1
    val = torch.randint(1, 4, (nnz,), generator=gen, device=dev()).float()
    g = G.CSRGraph(rowptr, col, val, n, n, split=SPLIT)
    assert g.n_items == n + 2 and g.n_long == 1 and int(g.long_rows[0, 0]) == n - 1
    X = torch.randint(-8, 9, (n, d), generator=gen, device=dev(), dtype=torch.float32)
    P = torch.randint(-8, 9, (n, d), generator=gen, device=dev(), dtype=torch.float32)
    b = torch.randint(-8, 9, (d,), generator=gen, device=dev(), dtype=torch.float32)
    assert X.numel() * 4 > 2 ** 32
    rows = torch.repeat_interleave(torch.arange(n, device=dev()), deg)
    Z = X.index_select(0, col[:n - 1]).mul_(val[:n - 1, None])        # rows 0 .. n-2 have one entry each
    Z = torch.cat([Z, torch.zeros(1, d, device=dev())])
    Z.index_add_(0, rows[n - 1:], X.index_select(0, col[n - 1:]) * val[n - 1:, None])
    Z += b
    want2 = (2.0 * X) * (Z > 0)
    want = P + (-0.5) * Z.clamp_min_(0)
    del Z, rows
    with profile() as widths:
        Y, Y2 = ops.spmm(g, X, bias=b, relu=True, out=P, pre_terms=[(1.0, P)], alpha=-0.5, cot_terms=[(2.0, X)])
    assert_route("tg", g, d, widths)
    assert Y.data_ptr() == P.data_ptr()
    assert torch.equal(Y2, want2), "Y2 differs, first row %d" % int(torch.nonzero((Y2 != want2).any(1))[0])
    assert torch.equal(Y, want), "Y differs, first row %d" % int(torch.nonzero((Y != want).any(1))[0])
    assert bool((Y2[n - 1] != 0).any())
    del X, P, Y, Y2, want, want2, g
    torch.cuda.empty_cache()
    print("operands beyond 4 GiB: %.1f s" % (time.time() - t0))


# -- rounding behaviour: float data against the derived running-sum bound -------------------------------------------
@gpu
@pytest.mark.parametrize("kind,d,route", ROUNDING, ids=["%s-%d-%s" % c for c in ROUNDING])
def test_rounding_within_the_running_sum_bound(kind, d, route):
    """Exact integers cannot notice reduced-precision accumulation or operands squeezed through a narrower type; these
    inputs can.  The bars are derived, not measured (rounding_problem() has the argument for Z):

        Y  = sum c_j p_j + alpha K:  |alpha| * bound_Z + 2^-23 * (n_pre + 2) * (sum |c_j| |p_j| + |alpha K|)
             (n_pre multiply-adds of the pre-terms and the one that joins alpha K; relu is 1-Lipschitz),
        Y2 = (sum c_j g_j) [Z > 0]:  2^-23 * n_cot * sum |c_j| |g_j|, compared where |Z64| exceeds bound_Z
             (elsewhere the sign of the computed Z is not determined; that share is capped at 1e-4 by the CPU test),
        Y3 = sum c3_j g_j:           2^-23 * n_cot * sum |c3_j| |g_j|.

    The graphs have split rows, so the finishing kernels are under the same bound row by row."""
    from graph_odenet_amd import ops
    g = gpu_graph(kind, "float")
    n = g.n_rows
    X, b, Z, bZ = rounding_problem(kind, d)
    gen = torch.Generator().manual_seed(5 + d)
    pre = [(c, torch.randn(n, d, generator=gen)) for c in PRE_C]
    cot = [(c, torch.randn(n, d, generator=gen)) for c in COT_C]
    Xd, bd = X.to(dev()), b.to(dev())

    def worst(got, want, bound, what, where=None):
        excess = (got.detach().cpu().double() - want).abs() - bound
        if where is not None:
            excess = excess[where]
        ratio = ((got.detach().cpu().double() - want).abs() / bound.clamp_min(1e-300))
        ratio = ratio[where] if where is not None else ratio
        print("%s %s d=%d: largest error / bound = %.3f" % (what, kind, d, float(ratio.max())))
        assert float(excess.max()) <= 0.0, "%s: %d elements beyond the bound, worst ratio %.3f" % (
            what, int((excess > 0).sum()), float(ratio.max()))

    with profile() as widths:
        Zg = ops.spmm(g, Xd, bias=bd)
    assert_route(route, g, d, widths)
    worst(Zg, Z, bZ, "Z")

    K = Z.clamp_min(0)
    Yr, Y2r, Y3r, _ = reference(Z, None, True, ALPHA_R, pre, cot, COT3_C)              # Z holds the bias already
    Y3 = torch.full((n, d), float("nan"), device=dev())
    Y, Y2 = ops.spmm(g, Xd, bias=bd, relu=True, alpha=ALPHA_R, pre_terms=[(c, t.to(dev())) for c, t in pre],
                     cot_terms=[(c, t.to(dev())) for c, t in cot], cot_out=Y3, cot_out_coefs=COT3_C)
    bY = abs(ALPHA_R) * bZ + U2 * (len(pre) + 2) * (sum(abs(c) * t.double().abs() for c, t in pre) + (ALPHA_R * K).abs())
    worst(Y, Yr, bY, "Y")
    clear = Z.abs() > bZ
    assert float((~clear).double().mean()) <= 1e-4
    worst(Y2, Y2r, U2 * len(cot) * sum(abs(c) * t.double().abs() for c, t in cot), "Y2", clear)
    worst(Y3, Y3r, U2 * len(cot) * sum(abs(c3) * t.double().abs() for c3, (_, t) in zip(COT3_C, cot)), "Y3")
