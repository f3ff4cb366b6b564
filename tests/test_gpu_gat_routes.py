"""Every kernel route and width of the one-head edge-attention family (csrc/edge.hip) against a float64 restatement.

Each case calls the ops wrappers directly on Ps, Pt, A2 (gat_logits, gat_agg_fwd, gat_agg_bwd - the first piece of gat_vjp -,
gat_scatter / the source-side SpMM, gat_maxpath_), first asserts that the route queries name the kernel the case is meant
for, and then compares w, den, out, dz, da, dPs, dPt and dA2 one by one with tests/gat_routes_design.py's restatement
(float64, index_add only, independent of the library and of oracle/).

Metric.  Errors are relative to the ROW's own scale, not to the global maximum: a per-edge array is scaled by the largest
|ref| among the edges of the same row of Mtgt, a per-node array by the row's own largest |ref|, and rows whose reference is
all zero (nodes without edges, the inactive rows of L among them) must be exactly zero.  da and dA2 are sums that cancel -
analytically da is 0 on a one-edge row and on a row whose edges share a source node, and the sum of a row's da is 0 - so
their scale is the cancellation-free magnitude val w (sum_c |dA_c y_c| + |dsum|) (per row / summed per node) that bounds
the rounding error of that sum; |da| never exceeds it.  dPs and dPt are sums of signed dz rows: a row that cancelled below
1/16 of its terms is measured against that sixteenth (gat_routes_design.node_error says why: at o = 1 fp32 arithmetic
alone is 4e-4 away under the unfloored metric).

Bound.  2e-5, the bound of this family in test_gpu_gat_qc.py: a float32 restatement of the reference stays within 2.1e-6
of float64 under this metric, so the bound is about 10 x what fp32 arithmetic alone costs, and every edge carries at least
1e-4 of its row's denominator (test_gat_routes.py), five times the bound: a dropped or doubled edge cannot hide.

Exact parts (logits, max path, scatter) use integer data and are compared bit for bit.

GAT_ROUTES_ERRORS=<file>: the worst error per route and quantity of the run is written there (profiles/gat_routes_errors.txt).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gat_routes_design as D                                           # noqa: E402

gpu = pytest.mark.gpu
SENT = 77.0
FORMS = (0, 1, 3, D.MAX_TERMS)                                           # dout, and cotangent combinations of 1, 3, 8 terms
PF_LPR = {4: 1, 8: 2, 16: 4, 32: 8, 64: 16}
REC_LPR = {16: 4, 32: 8, 64: 16, 128: 32, 256: 64}
FAMILY = {1: "PF", 2: "WAVE", 3: "GROUP", 4: "REC"}
ERRORS = {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def maxc(o):
    return 1 if o <= 64 else 2 if o <= 128 else 4 if o <= 256 else 8


def code(family, form=0):
    return family | (form << 8)


def scatter_code(o):
    return code(1, PF_LPR[o]) if o in PF_LPR else code(2, maxc(o))


@pytest.fixture(scope="module", autouse=True)
def errors_file():
    yield
    path = os.environ.get("GAT_ROUTES_ERRORS")
    if path and ERRORS:
        with open(path, "w") as f:
            f.write("# worst error per route and quantity, relative to the row's own scale (bound %g)\n" % D.TOL)
            for (route, q), e in sorted(ERRORS.items()):
                f.write("%-12s %-4s %.3e\n" % (route, q, e))


@functools.lru_cache(maxsize=None)
def edge_graph(kind, canonical=True, pattern=False, split=None):
    from graph_odenet_amd.gat_layers import EdgeGraph
    from graph_odenet_amd.graph import CSRGraph, from_coo
    d = D.design(kind, canonical, pattern)
    t = lambda x, dt=torch.int64: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev())
    vals = None if d.vals is None else t(d.vals, torch.float32)
    eg = EdgeGraph(t(d.src, torch.int32), t(d.tgt, torch.int32), from_coo(t(d.rows), t(d.cols), vals, d.n, d.E))
    assert eg.canonical == canonical
    assert torch.equal(eg.src.cpu().long(), torch.from_numpy(d.src)) and torch.equal(eg.tgt.cpu().long(), torch.from_numpy(d.tgt))
    assert (eg.Mt.val is None) == pattern
    if split is not None:                                                # the record list rebuilt with short records
        eg.Mt = CSRGraph(eg.Mt.rowptr, eg.Mt.col, eg.Mt.val, d.n, d.E, split=split)
        assert eg.Mt.n_long == 13 and eg.Mt.n_slots == sum(-(-x // split) for x in D.SHORT + D.LONG if x > split)
    else:
        assert eg.Mt.n_long == 0
    eg.act = t(d.act)
    eg.inactive = torch.ones(d.n, dtype=torch.bool, device=dev())
    eg.inactive[eg.act] = False
    return eg


def full(compact, eg, n):
    x = torch.zeros((n,) + tuple(compact.shape[1:]), dtype=torch.float32, device=dev())
    x[eg.act] = compact.to(dev())
    return x


def sentinel(*shape, offset=0):
    buf = torch.full((int(np.prod(shape)) + offset,), SENT, dtype=torch.float32, device=dev())
    return buf[offset:].view(*shape)


class Check:
    """Collects every figure of a case, prints it, and fails at the end: one run reports all quantities."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def add(self, route, q, err, exact):
        key = ("%s/%d" % (FAMILY[route & 255], route >> 8), q)
        ERRORS[key] = max(ERRORS.get(key, 0.0), err)
        print("%s %s %-4s err %.3e zero rows exact %s" % (self.case, key[0], q, err, exact))
        if not (err <= D.TOL and exact):
            self.bad.append((key, err, exact))

    def true(self, cond, what):
        if not cond:
            print("%s FAILED: %s" % (self.case, what))
            self.bad.append(what)

    def done(self):
        assert not self.bad, (self.case, self.bad)


def run_case(kind, o, canonical=True, pattern=False, split=None, offset=0, forms=FORMS, fwd_route=None, bwd_route=None):
    """One width on one graph through logits, forward, every backward form and the node sums.  fwd_route: the expected code;
    bwd_route(terms): likewise."""
    from graph_odenet_amd import ops
    d, v = D.design(kind, canonical, pattern), D.values(kind, canonical, o)
    eg = edge_graph(kind, canonical, pattern, split)
    n, E = d.n, d.E
    case = "%s%s%s o=%d" % (kind, "" if canonical else " non-canonical", " pattern" if pattern else "", o)
    ck = Check(case)
    Ps, Pt, A2 = full(v.Ps, eg, n), full(v.Pt, eg, n), full(v.A2, eg, n)
    bf, bw = v.bf.to(dev()), v.bw.to(dev())
    proj = ops.gat_proj(Ps, Pt, A2)
    a, amax = sentinel(E), sentinel(1)
    ops.gat_logits(proj, bw, eg.src, eg.tgt, a, amax)
    ref = D.reference(d, v)
    ck.true(torch.equal(a.cpu(), ref.a32) and amax.item() == ref.amax.item(), "logits bit for bit")
    out, w, den = sentinel(n, o, offset=offset), sentinel(E), sentinel(n)
    rt = ops.gat_agg_fwd_route(eg, proj, o, bf, a, amax, D.EPS, out, w, den)
    assert rt == fwd_route, (case, "forward route", rt, fwd_route)
    ops.gat_agg_fwd(eg, proj, o, bf, a, amax, D.EPS, out, w, den)
    for q, res in D.compare_forward(ref, w.cpu(), den[eg.act].cpu(), out[eg.act].cpu()).items():
        ck.add(rt, q, *res)
    ck.true(bool((out[eg.inactive] == 0).all()) and bool((den[eg.inactive] == np.float32(D.EPS)).all()), "rows without edges: out 0, den eps")
    for terms in forms:
        if terms:
            ref = D.reference(d, v, terms)
        cot = [(cf, full(ct, eg, n)) for cf, ct in zip(v.coef[:terms], v.cot[:terms])] if terms else None
        dout = None if terms else full(v.dout, eg, n)
        dz, da, dPs, dPt, dA2 = sentinel(E, o), sentinel(E), sentinel(n, o), sentinel(n, o), sentinel(n, 2)
        kw = dict(dPt=dPt, dA2=dA2, dout=dout, cot_terms=cot, cot_scale=v.cot_scale)
        rt = ops.gat_agg_bwd_route(eg, proj, o, bf, w, den, out, dz, da, **kw)
        assert rt == bwd_route(terms), (case, "backward route", terms, rt, bwd_route(terms))
        did = ops.gat_agg_bwd(eg, proj, o, bf, w, den, out, dz, da, **kw)
        assert did == ((rt & 255) == 4), (case, "did_target_sums", did, rt)
        if did:                                                           # the source side is two incidence products
            ops.spmm(eg.Ms_inc, dz, out=dPs)
            ops.spmm(eg.Ms_inc, da.view(-1, 1), out=dA2[:, 0:1])
        else:
            assert ops.gat_scatter_route(eg.Ms_inc, eg.Mt_inc, dz, da, dPs, dPt, dA2) == scatter_code(o), (case, "scatter route")
            ck.true(bool((dPt == SENT).all()) and bool((dA2 == SENT).all()), "dPt / dA2 untouched off the record route")
            ops.gat_scatter(eg.Ms_inc, eg.Mt_inc, dz, da, dPs, dPt, dA2)
        for q, res in D.compare_backward(ref, dz.cpu(), da.cpu(), dPs[eg.act].cpu(), dPt[eg.act].cpu(), dA2[eg.act].cpu()).items():
            ck.add(rt, q, *res)
        ck.true(all(bool((x[eg.inactive] == 0).all()) for x in (dPs, dPt, dA2)), "node sums of rows without edges are 0")
        del cot, dout, dz, da, dPs, dPt, dA2
    ck.done()


# ---- the routes ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("o", [4, 8, 16, 32, 64])
def test_prefetched_route(o):
    run_case("S", o, fwd_route=code(1, PF_LPR[o]), bwd_route=lambda terms: code(1, PF_LPR[o]))


@gpu
@pytest.mark.parametrize("o", [1, 2, 7, 12, 24, 48, 73, 128, 200, 256, 260, 512])
def test_wave_route(o):
    run_case("S", o, fwd_route=code(2, maxc(o)), bwd_route=lambda terms: code(2, maxc(o)))


@gpu
def test_wave_route_is_the_unaligned_fallback_of_the_prefetched_one():
    """o = 16 with `out` one float off a 16-byte boundary: forward and backward fall back to the wave kernels (the scatter,
    whose arrays are aligned, stays prefetched)."""
    run_case("S", 16, offset=1, fwd_route=code(2, 1), bwd_route=lambda terms: code(2, 1))


@gpu
@pytest.mark.parametrize("o", [7, 8, 24, 73, 200, 260, 512])
def test_group_route(o):
    """Above 65 536 rows and off the record set: a lane group per row; the cotangent-combining backward has no lane-group
    form and runs the wave kernel."""
    run_case("L", o, fwd_route=code(3, maxc(o)), bwd_route=lambda terms: code(2 if terms else 3, maxc(o)))


@gpu
@pytest.mark.parametrize("o", [24, 200])
def test_wave_backward_above_the_threshold(o):
    run_case("L", o, forms=(1, 3, D.MAX_TERMS), fwd_route=code(3, maxc(o)), bwd_route=lambda terms: code(2, maxc(o)))


@gpu
@pytest.mark.parametrize("o", [16, 32, 64, 128, 256])
def test_record_route_with_split_rows(o):
    run_case("L", o, split=D.SPLIT, fwd_route=code(4, REC_LPR[o]), bwd_route=lambda terms: code(4, REC_LPR[o]))


@gpu
def test_record_route_without_split_rows():
    run_case("L", 64, fwd_route=code(4, 16), bwd_route=lambda terms: code(4, 16))


@gpu
@pytest.mark.parametrize("kind,o,split,family", [("S", 16, None, 1), ("S", 73, None, 2), ("L", 24, None, 3), ("L", 32, D.SPLIT, 4)])
def test_pattern_only_variant(kind, o, split, family):
    form = {1: PF_LPR.get(o), 4: REC_LPR.get(o)}.get(family) or maxc(o)
    run_case(kind, o, pattern=True, split=split, fwd_route=code(family, form),
             bwd_route=lambda terms: code(2 if family == 3 and terms else family, form))


@gpu
@pytest.mark.parametrize("kind,o,family", [("S", 8, 1), ("S", 64, 1), ("S", 73, 2), ("S", 200, 2), ("L", 16, 3), ("L", 73, 3)])
def test_non_canonical_variant(kind, o, family):
    """Mtgt rows that disagree with tgt: `col` is present (no record route above the threshold, even at o = 16) and an
    edge's Pt row is not its row's."""
    form = PF_LPR[o] if family == 1 else maxc(o)
    run_case(kind, o, canonical=False, fwd_route=code(family, form),
             bwd_route=lambda terms: code(2 if family == 3 and terms else family, form))


@gpu
@pytest.mark.parametrize("kind", ["B0", "B1"])
def test_row_threshold_boundary(kind):
    """65 536 rows: the last size of the prefetched / wave kernels; 65 537: the first of the records."""
    rt = code(1, 4) if kind == "B0" else code(4, 4)
    run_case(kind, 16, split=D.SPLIT if kind == "B1" else None, forms=(0, 3), fwd_route=rt, bwd_route=lambda terms: rt)


# ---- exact parts --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("E,family", [(32_768, 5), (32_769, 6), (262_144 + 77, 6)])
def test_logits_bit_for_bit(E, family):
    """a = (as[src] + at[tgt]) + bw in fp32 and its maximum; the maximum sits in the last edge (the second trip of the
    grid-stride loop at E > 262 144)."""
    from graph_odenet_amd import ops
    rs = np.random.RandomState(E)
    n = 1000
    A2 = torch.from_numpy(rs.uniform(-1, 1, (n, 2)).astype(np.float32))
    A2[n - 1, 0] = 5.0
    src, tgt = torch.from_numpy(rs.randint(0, n - 1, E)), torch.from_numpy(rs.randint(0, n, E))
    src[E - 1] = n - 1
    bw = torch.tensor([-0.625])
    want = (A2[src, 0] + A2[tgt, 1]) + bw[0]
    assert want.argmax().item() == E - 1
    P = torch.zeros(n, 4, device=dev())
    proj = ops.gat_proj(P, P, A2.to(dev()))
    a, amax = sentinel(E), sentinel(1)
    s32, t32 = src.int().to(dev()), tgt.int().to(dev())
    assert ops.gat_logits_route(proj, bw.to(dev()), s32, t32, a, amax) == code(family)
    ops.gat_logits(proj, bw.to(dev()), s32, t32, a, amax)
    assert torch.equal(a.cpu(), want) and amax.item() == want.max().item()


def maxpath_inputs(E, ties):
    rs = np.random.RandomState(E)
    a = torch.from_numpy(rs.uniform(-3, 3, E).astype(np.float32))
    a[list(ties)] = 4.0
    da = torch.from_numpy(rs.randint(-8, 9, E).astype(np.float32))
    return a, da


@gpu
@pytest.mark.parametrize("E,family,ties", [(32_768, 5, (11_000, 11_000 + 1024 * 7 - 3, 32_767)), (32_769, 6, (20_000, 32_768)),
                                          (40_000, 6, (13_000, 29_000, 39_999))])
def test_maxpath_bit_for_bit_and_first_tie_takes_the_path(E, family, ties):
    """da is integer-valued, so every partial sum is an fp32 integer and the result does not depend on the order.  The
    maximum is attained several times (at E = 40 000 in blocks 3, 7 and 9 of the two-stage route): the FIRST edge takes it."""
    from graph_odenet_amd import ops
    a, da = maxpath_inputs(E, ties)
    want = da.clone()
    want[min(ties)] -= da.double().sum().float()
    ga, gda, gmax = a.to(dev()), da.to(dev()), torch.tensor([4.0], device=dev())
    assert ops.gat_maxpath_route(ga, gmax, gda) == code(family)
    ops.gat_maxpath_(ga, gmax, gda)
    assert torch.equal(gda.cpu(), want)


@gpu
@pytest.mark.parametrize("E,ties", [(20_000, (7_000, 15_000)), (40_000, (13_000, 29_000, 39_999))])
def test_maxpath_corrects_the_target_sums(E, ties):
    """With dat (target-side sums formed before the correction: the record route) even E <= 32 768 takes the two-stage
    route, and dat[tgt[e*]] loses the same amount; nothing else of dat, and nothing of the source column, changes."""
    from graph_odenet_amd import ops
    a, da = maxpath_inputs(E, ties)
    n = 500
    tgt = torch.from_numpy(np.random.RandomState(E + 1).randint(0, n, E))
    dA2 = torch.zeros(n, 2)
    dA2[:, 1].index_add_(0, tgt, da)
    dA2[:, 0] = torch.arange(n) % 17
    S = da.double().sum().float()
    want_da, want_A2 = da.clone(), dA2.clone()
    want_da[min(ties)] -= S
    want_A2[tgt[min(ties)], 1] -= S
    ga, gda, gmax, gA2, gt = a.to(dev()), da.to(dev()), torch.tensor([4.0], device=dev()), dA2.to(dev()), tgt.int().to(dev())
    dat = gA2.view(-1)[1:]
    assert ops.gat_maxpath_route(ga, gmax, gda, gt, dat, 2) == code(6)
    ops.gat_maxpath_(ga, gmax, gda, gt, dat, 2)
    assert torch.equal(gda.cpu(), want_da) and torch.equal(gA2.cpu(), want_A2)
    assert S.item() != 0


@gpu
@pytest.mark.parametrize("kind", ["S", "L"])
@pytest.mark.parametrize("o", [4, 8, 16, 32, 64, 7, 73, 200, 260, 512])
def test_scatter_bit_for_bit(kind, o):
    """Integer dz and da: both incidence sums against index_add, bit for bit, on every prefetched form and every MAXC; row 0,
    the last row and the isolated nodes included; outputs pre-filled so that an unwritten element shows."""
    from graph_odenet_amd import ops
    d, eg = D.design(kind), edge_graph(kind)
    rs = np.random.RandomState(o)
    dz = torch.from_numpy(rs.randint(-8, 9, (d.E, o)).astype(np.float32))
    da = torch.from_numpy(rs.randint(-8, 9, d.E).astype(np.float32))
    s, t = torch.from_numpy(d.lut[d.src]), torch.from_numpy(d.lut[d.tgt])
    na = d.act.size
    want = [torch.zeros(na, o).index_add_(0, i, dz) for i in (s, t)]
    want_a = torch.stack([torch.zeros(na).index_add_(0, i, da) for i in (s, t)], 1)
    assert max(x.abs().max().item() for x in want) <= 8 * 1000                   # fp32 integers
    gdz, gda = dz.to(dev()), da.to(dev())
    dPs, dPt, dA2 = sentinel(d.n, o), sentinel(d.n, o), sentinel(d.n, 2)
    assert ops.gat_scatter_route(eg.Ms_inc, eg.Mt_inc, gdz, gda, dPs, dPt, dA2) == scatter_code(o)
    ops.gat_scatter(eg.Ms_inc, eg.Mt_inc, gdz, gda, dPs, dPt, dA2)
    assert torch.equal(dPs[eg.act].cpu(), want[0]) and torch.equal(dPt[eg.act].cpu(), want[1])
    assert torch.equal(dA2[eg.act].cpu(), want_a)
    assert all(bool((x[eg.inactive] == 0).all()) for x in (dPs, dPt, dA2))
    assert 0 in d.act and d.n - 1 in d.act and (kind == "S" or bool(eg.inactive.any()))
