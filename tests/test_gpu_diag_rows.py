"""Option diag_rows: rows that hold their diagonal only leave SpMM launches of the rk4 solves (csrc/spmm.hip: epilogue
fields Y2_scale / Y2_scaled / n_items_full; csrc/gemm_pc.hip: the DIAG form of gn_gemm_fwd_pc_kernel behind
gode_gn_time_gemm_diag_f32; csrc/ode_driver.hip: stages 0-2 of gode_gcn_ode_rk4_forward, the one-pass branch of
gode_gcn_ode_rk4_adjoint; gcn_ode.tuned_graph: the gate).

Adjoint: for a row i whose only entry in A and in A^T is its own non-zero diagonal, (A^T dZ)[i] = a_ii dZ[i] and no other
row of the product gathers dZ[i]: the launch that forms dZ stores fmaf(a_ii, dZ[i], 0) into dS - the multiply-add the
product's one-entry record does - and the product runs on A^T's record list without those rows.  Forward: for a row
whose only entry in A is its diagonal the dense launch stores relu(a_ii S[i] + b) itself and the SpMM runs on A's list
without it; S[i] is not stored where the row is isolated (nobody gathers it).  Every comparison is torch.equal, option 1
against option 0 in one process.

The graph: 65 610 rows (the smallest count that reaches the large route is 65 537; the last 32-row tile is partial),
d = 128, 4 channels per GroupNorm group, values NOT normalised (diagonals .25 .. 1.0, .37 on the rows flagged on one side
only), so no scale is 1.0.  Every third row is isolated, so isolated and ordinary rows alternate inside every 32-row tile
of the dense launches, and the one-entry records of the SpMM (isolated rows, rows flagged on one side only, the
off-diagonal single entry, the stored 0.0) share 256-thread blocks.  One row each: above 256 entries in A (split), above
256 entries in A^T, empty, a single entry off the diagonal, diagonal-only with a stored 0.0; 1 367 rows flagged in A
only and at least as many in A^T only (their dZ row is gathered, or their dS row needs A^T's full row: neither may be treated as isolated).
"""
import ctypes

import pytest
import torch

from test_gpu_rk_close_once import dev, options, profiled

pytestmark = pytest.mark.gpu

N, D, STEPS = 65_610, 128, 2
EMPTY, OFFD, ZERO, LONG, LONGT = 10, 13, 15, 5, 7


def build_graph():
    from graph_odenet_amd import graph as G
    gen = torch.Generator().manual_seed(65_610)
    ar = torch.arange(N)
    ordinary = ar[ar % 3 != 0]
    a_only = (ar % 48 == 1)                    # their row of A is the diagonal alone, their column is not
    at_only = (ar % 48 == 2)                   # their column of A is the diagonal alone, their row is not
    no_row = a_only.clone()
    no_row[[EMPTY, OFFD]] = True
    r = ordinary.repeat_interleave(5)
    c = ordinary[torch.randint(0, ordinary.numel(), (r.numel(),), generator=gen)]
    pick = ordinary[(ordinary > 100) & ~at_only[ordinary] & ~no_row[ordinary]][:600:2]
    assert pick.numel() == 300
    ao, to = ar[a_only], ar[at_only]
    # (i + 3, i): somebody gathers every row flagged in A only;  (i, i + 2): every row flagged in A^T only gathers
    r = torch.cat([r, torch.full((300,), LONG), pick, ao + 3, to, torch.tensor([OFFD])])
    c = torch.cat([c, pick, torch.full((300,), LONGT), ao, to + 2, torch.tensor([OFFD + 1])])
    keep = (r != c) & ~no_row[r] & ~at_only[c]
    keep[-1] = True                                                   # (OFFD, OFFD + 1): the row's one entry
    diag_rows = ar[(ar != EMPTY) & (ar != OFFD)]
    key = torch.unique(torch.cat([r[keep], diag_rows]) * N + torch.cat([c[keep], diag_rows]))
    r, c = key // N, key % N
    v = torch.rand(key.numel(), generator=gen) * 2 - 1
    on = r == c
    v[on] = 0.25 + 0.125 * (r[on] % 7).float()
    v[on & (a_only | at_only)[r]] = 0.37
    v[on & (r == ZERO)] = 0.0
    g = G.from_coo(r.to(dev()), c.to(dev()), v.to(dev()), N, N, split=256, coalesce=False)   # 256: the large graphs' split
    return g, a_only, at_only


@pytest.fixture(scope="module")
def graph():
    g, a_only, at_only = build_graph()
    gt = g.transpose()
    ar = torch.arange(N)
    fa, ft, iso = (x.diag.cpu() != 0 for x in (g.diag_rows(), gt.diag_rows(), gt.isolated_rows()))
    want_iso = (ar % 3 == 0) & (ar != ZERO)
    assert torch.equal(iso, want_iso) and torch.equal(fa & ft, iso) and 3 * int(iso.sum()) > N - 9
    # (some more rows are flagged in A^T only: ordinary rows that none of the random entries happens to gather)
    assert torch.equal(fa & ~ft, a_only) and bool((ft & ~fa)[at_only].all()) and int(a_only.sum()) == int(at_only.sum()) == 1367
    assert g.n_long == 1 and int(g.long_rows[0, 0]) == LONG and gt.n_long == 1 and int(gt.long_rows[0, 0]) == LONGT
    rp = g.rowptr.cpu()
    assert rp[EMPTY + 1] == rp[EMPTY] and rp[OFFD + 1] - rp[OFFD] == 1 and int(g.col[rp[OFFD]]) == OFFD + 1
    assert rp[ZERO + 1] - rp[ZERO] == 1 and int(g.col[rp[ZERO]]) == ZERO and float(g.val[rp[ZERO]]) == 0.0
    assert float(gt.isolated_rows().diag.max()) == 1.0 and float(gt.isolated_rows().diag[3]) == 0.25 + 0.125 * 3
    return g, iso.to(dev())


def _spmm(g, items, n_items, X, Y, ep):
    from graph_odenet_amd import _lib
    rc = _lib.load().gode_spmm_csr_f32(_lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val), _lib.ptr(items), n_items,
                                       _lib.ptr(g.long_rows), g.n_long, _lib.ptr(g.partial(D)), _lib.ptr(X), D, _lib.ptr(Y), D,
                                       g.n_rows, D, ctypes.byref(ep) if ep is not None else None, _lib.stream_ptr())
    return rc


def test_launches_scaled_rows_and_core_list(graph):
    """Sp(cotangent; scale -> dS) + SpT(core list) against Sp(cotangent) + SpT(full list): the same k, the same dZ on the
    rows that are not isolated, the same dS, the same per-block column sums.  dS starts as NaN everywhere (every row is
    stored by exactly one of the two launches) and the isolated rows of dZ start as NaN and stay NaN: nothing stores them
    and nothing reads them."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    g, iso = graph
    gt = g.transpose()
    core = gt.isolated_rows()
    gen = torch.Generator(device=dev()).manual_seed(11)
    S, c0, c1 = (torch.randn(N, D, generator=gen, device=dev()) for _ in range(3))
    bias = torch.randn(D, generator=gen, device=dev())
    cot = [(0.5, c0), (-1.25, c1)]
    rows = int(lib.gode_spmm_y2_colsum_rows(g.n_items, g.n_long, D))
    assert rows > 0

    def run(scaled):
        k = torch.empty(N, D, device=dev())
        dZ = torch.zeros(N, D, device=dev())
        dS = torch.full((N, D), float("nan"), device=dev())
        colsum = torch.empty(rows, D, device=dev())
        ep = _lib.SpmmEpilogue()
        ep.bias, ep.relu, ep.alpha = bias.data_ptr(), 1, 1.0
        ep.cot = _lib.lincomb(cot)
        ep.Y2, ep.Y2_colsum = dZ.data_ptr(), colsum.data_ptr()
        if scaled:
            dZ[iso] = float("nan")
            ep.Y2_scale, ep.Y2_scaled = core.diag.data_ptr(), dS.data_ptr()
        assert _spmm(g, g.items, g.n_items, S, k, ep) == 0
        if scaled:
            pt = _lib.SpmmEpilogue()
            pt.alpha, pt.n_items_full = 1.0, gt.n_items
            assert _spmm(gt, core.items, core.n_items, dZ, dS, pt) == 0
        else:
            assert _spmm(gt, gt.items, gt.n_items, dZ, dS, None) == 0
        torch.cuda.synchronize()
        return k, dZ, dS, colsum

    k0, dZ0, dS0, cs0 = run(False)
    k1, dZ1, dS1, cs1 = run(True)
    assert torch.isfinite(dS0).all() and torch.isfinite(dZ0).all() and dS0[iso].abs().max().item() > 0
    assert torch.equal(k1, k0)
    assert torch.equal(dZ1[~iso], dZ0[~iso]) and torch.isnan(dZ1[iso]).all()
    assert torch.equal(dS1, dS0)
    assert torch.equal(cs1, cs0)
    # the fields come as a pair, with a cotangent output
    ep = _lib.SpmmEpilogue()
    ep.alpha, ep.cot, ep.Y2, ep.Y2_scale = 1.0, _lib.lincomb(cot), dZ0.data_ptr(), core.diag.data_ptr()
    assert _spmm(g, g.items, g.n_items, S, k0, ep) != 0
    ep = _lib.SpmmEpilogue()
    ep.alpha, ep.Y2_scale, ep.Y2_scaled = 1.0, core.diag.data_ptr(), dS0.data_ptr()
    assert _spmm(g, g.items, g.n_items, S, k0, ep) != 0


class _Problem:
    def __init__(self, g):
        from graph_odenet_amd import models, odeint as OI
        torch.manual_seed(7)
        f = models.ODEfunc(D)
        with torch.no_grad():
            f.norm1.weight.uniform_(0.5, 1.5)
            f.norm1.bias.uniform_(-0.5, 0.5)
        f = f.to(dev())
        f.set_adj(g)
        gen = torch.Generator().manual_seed(D)
        self.y0 = torch.randn(N, D, generator=gen).to(dev())
        self.a1 = torch.randn(N, D, generator=gen).to(dev())
        self.fwd, self.mk_adj, _ = OI._fields(f, self.y0)
        assert getattr(self.fwd, "rk4_native", None) is not None and getattr(self.fwd, "row_order", None) is None
        info = g.__dict__["_tuned_info"][(D, "auto")]
        assert info["core_lists"] and 3 * info["isolated_rows"] > N - 9          # the gate took the list
        with torch.no_grad():
            y = [self.y0.clone()]
            self.fwd.rk4_native(y, 0.0, 1.0, STEPS)
        self.y1 = y[0]

        self.f = f

    def forward(self):
        with torch.no_grad():
            y = [self.y0.clone()]
            with profiled() as launches:
                self.fwd.rk4_native(y, 0.0, 1.0, STEPS)
        return y[0], launches

    def adjoint(self, iso):
        """A 2-step adjoint solve from y(1); the isolated rows of the workspace's dZ are NaN before it.
        -> (y, a, theta), profiled launches, whether those rows are still NaN afterwards."""
        with torch.no_grad():
            adj = self.mk_adj()
            comps = adj.new_state(self.y1)
            comps[1].copy_(self.a1)
            dZ = adj.w.bwd()[0]
            dZ.zero_()
            dZ[iso] = float("nan")
            with profiled() as launches:
                adj.rk4_native(comps, 1.0, 0.0, STEPS)
            res = (comps[0].clone(), comps[1].clone(), adj.theta.clone())
            return res, launches, bool(torch.isnan(dZ[iso]).all()), bool(torch.isfinite(dZ[iso]).all())


@pytest.fixture(scope="module")
def problem(graph):
    return _Problem(graph[0])


@pytest.mark.parametrize("overlap", [1, 0])
def test_adjoint_solve_bit_identical_and_same_launch_list(graph, problem, overlap):
    """gode_gcn_ode_rk4_adjoint, 2 steps: y, a, theta with diag_rows 1 against 0 under both schedules, and the same
    profiled launch list (kinds and extra-array counts).  With the option on nobody writes or reads the isolated rows of
    dZ (they stay NaN and every result is finite); with it off the full list writes them."""
    iso = graph[1]
    out = {}
    for on in (1, 0):
        with options(diag_rows=on, overlap=overlap):
            out[on] = problem.adjoint(iso)
    for name, u, v in zip(("y", "a", "theta"), out[1][0], out[0][0]):
        assert torch.isfinite(u).all(), name
        assert torch.equal(u, v), "%s differs between diag_rows 1 and 0" % name
    assert out[1][0][2].abs().max().item() > 0 and not torch.equal(out[1][0][1], problem.a1)
    assert [(k & 0xff, e) for k, e in out[1][1]] == [(k & 0xff, e) for k, e in out[0][1]]
    assert [k for k, _ in out[1][1]] == [k for k, _ in out[0][1]]
    assert out[1][2] and not out[0][2] and out[0][3]


def test_full_list_when_the_one_pass_route_is_off(graph, problem):
    """bwd_wgrad 0: the other branch of the driver still reads dS on the side stream while Sp runs, so it keeps the full
    lists under diag_rows 1 - the isolated rows of dZ are written - and gives the bits of diag_rows 0."""
    iso = graph[1]
    out = {}
    for on in (1, 0):
        with options(diag_rows=on, bwd_wgrad=0):
            out[on] = problem.adjoint(iso)
    for u, v in zip(out[1][0], out[0][0]):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    assert out[1][3] and out[0][3]


def _lincomb_call(fn, terms, f, t, S, *more):
    from graph_odenet_amd import _lib
    lc = _lib.lincomb(terms)
    return fn(ctypes.byref(lc), N, D, f.norm1.num_groups, f.norm1.eps, _lib.ptr(f.norm1.weight), _lib.ptr(f.norm1.bias),
              _lib.ptr(f.gc1.weight), D, 1, t, _lib.ptr(S), *more, _lib.stream_ptr())


@pytest.mark.parametrize("n_terms", [1, 2, 3])
def test_launches_dense_diag_and_core_list(graph, problem, n_terms):
    """Gf(diag) + Sp(core list of A) against Gf + Sp(full list), bias + relu epilogue, 1 / 2 / 3 input terms (stages 0-2 of
    an rk4 step): the same k everywhere (k starts as NaN: every row is stored by exactly one of the two launches), the
    same S on the rows that are not isolated; the isolated rows of S start as NaN and stay NaN - not stored, not read."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    g, iso = graph
    f = problem.f
    a, skip = g.diag_rows(), g.transpose().isolated_rows().diag
    gen = torch.Generator(device=dev()).manual_seed(20 + n_terms)
    terms = [(c, torch.randn(N, D, generator=gen, device=dev())) for c in (1.0, 0.5, -0.25)[:n_terms]]
    bias = f.gc1.bias.detach()

    def sp(items, n_items, S, k):
        ep = _lib.SpmmEpilogue()
        ep.bias, ep.relu, ep.alpha, ep.n_items_full = bias.data_ptr(), 1, 1.0, g.n_items
        assert _spmm(g, items, n_items, S, k, ep) == 0

    with torch.no_grad():
        S0, k0 = torch.empty(N, D, device=dev()), torch.empty(N, D, device=dev())
        assert _lincomb_call(lib.gode_gn_time_gemm_f32, terms, f, 0.3, S0) == 0
        sp(g.items, g.n_items, S0, k0)
        S1 = torch.zeros(N, D, device=dev())
        S1[iso] = float("nan")
        k1 = torch.full((N, D), float("nan"), device=dev())
        taken = ctypes.c_int32(-1)
        assert _lincomb_call(lib.gode_gn_time_gemm_diag_f32, terms, f, 0.3, S1, _lib.ptr(a.diag), _lib.ptr(skip),
                             _lib.ptr(bias), _lib.ptr(k1), ctypes.byref(taken)) == 0
        assert taken.value == 1
        sp(a.items, a.n_items, S1, k1)
        torch.cuda.synchronize()
        assert torch.isfinite(k0).all() and k0[a.diag != 0].abs().max().item() > 0
        assert torch.equal(k1, k0)
        assert torch.equal(S1[~iso], S0[~iso]) and torch.isnan(S1[iso]).all()
        # the fp32-MFMA forward kernel has no such form: the plain launch is issued and says so
        with options(fwd_pc=0):
            S2 = torch.full((N, D), float("nan"), device=dev())
            k2 = torch.full((N, D), float("nan"), device=dev())
            taken = ctypes.c_int32(-1)
            assert _lincomb_call(lib.gode_gn_time_gemm_diag_f32, terms, f, 0.3, S2, _lib.ptr(a.diag), _lib.ptr(skip),
                                 _lib.ptr(bias), _lib.ptr(k2), ctypes.byref(taken)) == 0
            torch.cuda.synchronize()
            assert taken.value == 0 and torch.isfinite(S2).all() and torch.isnan(k2).all()


@pytest.mark.parametrize("fwd_pc", [3, 0])
def test_forward_solve_bit_identical_and_same_launch_list(problem, fwd_pc):
    """gode_gcn_ode_rk4_forward, 2 steps: y(1) with diag_rows 1 against 0 and the same profiled launch list - on the
    producer / consumer forward kernel (stages 0-2 take the DIAG form: the launch-level test above shows the launcher
    reporting it for these shapes) and with fwd_pc 0, where the driver falls back to the full list launch by launch."""
    out = {}
    for on in (1, 0):
        with options(diag_rows=on, fwd_pc=fwd_pc):
            out[on] = problem.forward()
    assert torch.isfinite(out[1][0]).all() and not torch.equal(out[1][0], problem.y0)
    assert torch.equal(out[1][0], out[0][0])
    assert out[1][1] == out[0][1] and len(out[1][1]) == 8 * STEPS
    if fwd_pc == 3:
        assert torch.equal(out[1][0], problem.y1)
