"""Option diag_last: the last stage of a forward rk4 step leaves the diagonal-only rows of A out of its SpMM as well
(csrc/gemm_pc.hip: gn_gemm_fwd_pc_kernel with AUX and DIAG behind gode_gn_time_gemm_diag_aux_f32; csrc/ode_driver.hip:
feval_large on the closing-combination-once route).

The product of that stage is y_new = P + alpha relu(A S + b), P the step's closing combination, read and overwritten in one
array.  For a row i whose only entry in A is its diagonal the dense launch stores
y_new[i] = fmaf(alpha, relu(fmaf(a_ii, S[i], 0) + b), P[i]) itself - the chain of the SpMM's one-entry record - with P[i]
handed from the launch's producer waves to its consumer waves through LDS; the producers store P only on the other rows,
and the SpMM runs on A's core list.  Every comparison is torch.equal against the plain launches in one process.

The graph: 66 021 rows (above 65 536; the last 32-row tile holds 5 rows), d = 128, values NOT normalised: diagonals
.25 .. .85 and .37 on the rows flagged on one side only, so no a_ii is 1.0.  Every third row is isolated, so flagged and
ordinary rows alternate inside every 32-row tile; 1 376 rows are flagged in A only (somebody gathers their S row) and as
many in A^T only (their row of A gathers); one row above 256 entries in A (split), one in A^T, one empty row, one row with
a single entry off the diagonal, one diagonal-only row with a stored 0.0.  A's whole list holds more than 65 536 records,
its core list fewer: n_items_full is what keeps the SpMM on the kernel of the whole list.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_rk_close_once import dev, options, profiled

pytestmark = pytest.mark.gpu

N, D, STEPS = 66_021, 128, 2
EMPTY, OFFD, ZERO, LONG, LONGT = 10, 13, 15, 5, 7
H = 0.5


def build_graph():
    from graph_odenet_amd import graph as G
    gen = torch.Generator().manual_seed(N)
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
    with_diag = ar[(ar != EMPTY) & (ar != OFFD)]
    key = torch.unique(torch.cat([r[keep], with_diag]) * N + torch.cat([c[keep], with_diag]))
    r, c = key // N, key % N
    v = torch.rand(key.numel(), generator=gen) * 2 - 1
    on = r == c
    v[on] = 0.25 + 0.1 * (r[on] % 7).float()
    v[on & (a_only | at_only)[r]] = 0.37
    v[on & (r == ZERO)] = 0.0
    g = G.from_coo(r.to(dev()), c.to(dev()), v.to(dev()), N, N, split=256, coalesce=False)   # 256: the large graphs' split
    return g, a_only, at_only


@pytest.fixture(scope="module")
def graph():
    g, a_only, at_only = build_graph()
    gt = g.transpose()
    ar = torch.arange(N)
    a = g.diag_rows()
    fa, ft, iso = (x.diag.cpu() != 0 for x in (a, gt.diag_rows(), gt.isolated_rows()))
    assert torch.equal(iso, (ar % 3 == 0) & (ar != ZERO)) and torch.equal(fa & ft, iso)
    assert torch.equal(fa & ~ft, a_only) and bool((ft & ~fa)[at_only].all()) and int(a_only.sum()) == int(at_only.sum()) == 1376
    assert g.n_long == 1 and int(g.long_rows[0, 0]) == LONG
    d = a.diag.cpu()[fa]
    assert float(d.max()) < 0.9 and float(d.min()) > 0.2 and not bool((d == 1.0).any())
    assert N > 65_536 and N % 32 == 5 and g.n_items > 65_536 and 0 < a.n_items < 65_536
    return g, fa.to(dev()), iso.to(dev())


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
        assert D // f.norm1.num_groups == 4
        gen = torch.Generator().manual_seed(D)
        self.y0 = torch.randn(N, D, generator=gen).to(dev())
        self.fwd, _, _ = OI._fields(f, self.y0)
        assert getattr(self.fwd, "rk4_native", None) is not None and getattr(self.fwd, "row_order", None) is None
        info = g.__dict__["_tuned_info"][(D, "auto")]
        assert info["core_lists"]                                                 # the gate took the lists
        self.f = f

    def forward(self, iso):
        """A 2-step forward solve; the isolated rows of the workspace's S are NaN before it.
        -> y(1), profiled launches, whether those rows are all NaN / all finite afterwards."""
        with torch.no_grad():
            y = [self.y0.clone()]
            S = self.fwd.w.S
            S.zero_()
            S[iso] = float("nan")
            with profiled() as launches:
                self.fwd.rk4_native(y, 0.0, 1.0, STEPS)
            return y[0], launches, bool(torch.isnan(S[iso]).all()), bool(torch.isfinite(S[iso]).all())


@pytest.fixture(scope="module")
def problem(graph):
    return _Problem(graph[0])


def _spmm(g, items, n_items, X, Y, ep):
    from graph_odenet_amd import _lib
    return _lib.load().gode_spmm_csr_f32(_lib.ptr(g.rowptr), _lib.ptr(g.col), _lib.ptr(g.val), _lib.ptr(items), n_items,
                                         _lib.ptr(g.long_rows), g.n_long, _lib.ptr(g.partial(D)), _lib.ptr(X), D, _lib.ptr(Y), D,
                                         g.n_rows, D, ctypes.byref(ep), _lib.stream_ptr())


@pytest.fixture(scope="module")
def stage_inputs():
    """The four arrays of a last stage, the stage's coefficients y + h (k0 - k1 + k2), those of the closing combination
    y + h/8 k0 + 3h/8 k1 + 3h/8 k2, and alpha = h b_3."""
    gen = torch.Generator(device=dev()).manual_seed(31)
    arrays = [torch.randn(N, D, generator=gen, device=dev()) for _ in range(4)]
    xc = [1.0, float(np.float32(H)), float(np.float32(-H)), float(np.float32(H))]
    ac = [1.0, float(np.float32(H / 8.0)), float(np.float32(3.0 * H / 8.0)), float(np.float32(3.0 * H / 8.0))]
    return arrays, xc, ac, float(np.float32(H / 8.0))


@pytest.mark.parametrize("cg", [4, 0])
def test_launch_pair_dense_last_and_core_list(graph, problem, stage_inputs, cg):
    """Gf(last stage: aux + diag) + Sp(core list of A) against Gf(aux) + Sp(full list), with and without GroupNorm.  `out` and S
    start as NaN.  After the dense launch alone `out` holds P of the plain launch on the rows A does not flag and the final
    y_new on the rows it flags; after the SpMM it is the plain pair's y_new everywhere - every row stored by exactly one of
    the two launches.  S is equal on the rows that are not isolated and still NaN on the isolated ones."""
    from graph_odenet_amd import _lib
    lib = _lib.load()
    g, fa, iso = graph
    f = problem.f
    a, skip = g.diag_rows(), g.transpose().isolated_rows().diag
    arrays, xc, ac, alpha = stage_inputs
    bias = f.gc1.bias.detach()
    groups = D // cg if cg else 0
    gamma, beta = (f.norm1.weight, f.norm1.bias) if cg else (None, None)
    coefs = (ctypes.c_float * 8)(*(ac + [0.0] * 4))

    def dense(fn, S, *more):
        lc = _lib.lincomb(list(zip(xc, arrays)))
        return fn(ctypes.byref(lc), N, D, groups, f.norm1.eps, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(f.gc1.weight), D, 1, 0.3,
                  _lib.ptr(S), *more, _lib.stream_ptr())

    def sp(items, n_items, S, out):
        ep = _lib.SpmmEpilogue()
        ep.bias, ep.relu, ep.alpha, ep.n_items_full = bias.data_ptr(), 1, alpha, g.n_items
        ep.pre = _lib.lincomb([(1.0, out)])
        assert _spmm(g, items, n_items, S, out, ep) == 0

    def nan():
        return torch.full((N, D), float("nan"), device=dev())

    with torch.no_grad():
        S0, out0 = nan(), nan()
        assert dense(lib.gode_gn_time_gemm_xout_aux_f32, S0, None, coefs, _lib.ptr(out0)) == 0
        P0 = out0.clone()
        sp(g.items, g.n_items, S0, out0)
        S1, out1 = nan(), nan()
        taken = ctypes.c_int32(-1)
        assert dense(lib.gode_gn_time_gemm_diag_aux_f32, S1, coefs, _lib.ptr(out1), alpha, _lib.ptr(a.diag), _lib.ptr(skip),
                     _lib.ptr(bias), ctypes.byref(taken)) == 0
        assert taken.value == 1
        mid = out1.clone()
        sp(a.items, a.n_items, S1, out1)
        torch.cuda.synchronize()
        assert torch.isfinite(P0).all() and torch.isfinite(out0).all() and torch.isfinite(S0).all()
        assert not torch.equal(out0[fa], P0[fa])                     # alpha relu(..) moves the flagged rows
        assert torch.equal(mid[~fa], P0[~fa])
        assert torch.equal(mid[fa], out0[fa])
        assert torch.equal(out1, out0)
        assert torch.equal(S1[~iso], S0[~iso]) and torch.isnan(S1[iso]).all()
        # the fp32-MFMA forward kernel has no such form: the plain launch with the second combination is issued and says so
        with options(fwd_pc=0):
            S2, out2 = nan(), nan()
            taken = ctypes.c_int32(-1)
            assert dense(lib.gode_gn_time_gemm_diag_aux_f32, S2, coefs, _lib.ptr(out2), alpha, _lib.ptr(a.diag), _lib.ptr(skip),
                         _lib.ptr(bias), ctypes.byref(taken)) == 0
            torch.cuda.synchronize()
            assert taken.value == 0 and torch.isfinite(S2).all() and torch.equal(out2, P0)
        # three terms: no kernel forms the second combination on this route - nothing is launched
        lc = _lib.lincomb(list(zip(xc[:3], arrays[:3])))
        S3, out3 = nan(), nan()
        taken = ctypes.c_int32(-1)
        assert lib.gode_gn_time_gemm_diag_aux_f32(ctypes.byref(lc), N, D, groups, f.norm1.eps, _lib.ptr(gamma), _lib.ptr(beta),
                                                  _lib.ptr(f.gc1.weight), D, 1, 0.3, _lib.ptr(S3), coefs, _lib.ptr(out3), alpha,
                                                  _lib.ptr(a.diag), _lib.ptr(skip), _lib.ptr(bias), ctypes.byref(taken),
                                                  _lib.stream_ptr()) == -5
        torch.cuda.synchronize()
        assert taken.value == 0 and torch.isnan(out3).all() and torch.isnan(S3).all()


def test_forward_solve_bit_identical_and_same_launch_list(graph, problem):
    """gode_gcn_ode_rk4_forward, 2 steps: y(1) with diag_last 1 against 0 under diag_rows 1, and against diag_rows 0 - the same
    bits and the same profiled launch list (kinds and extra-array counts).  With diag_last 1 no stage stores the isolated
    rows of S (NaN before, NaN after) and y(1) is finite; with diag_last 0 the last stage's plain launch stores them."""
    iso = graph[2]
    out = {}
    for key, (rows, last) in (("last", (1, 1)), ("stages", (1, 0)), ("off", (0, 1))):
        with options(diag_rows=rows, diag_last=last):
            out[key] = problem.forward(iso)
    y = out["last"][0]
    assert torch.isfinite(y).all() and not torch.equal(y, problem.y0)
    assert torch.equal(y, out["stages"][0]) and torch.equal(y, out["off"][0])
    assert out["last"][1] == out["stages"][1] == out["off"][1] and len(out["last"][1]) == 8 * STEPS
    assert out["last"][2] and out["stages"][3] and out["off"][3]


@pytest.mark.parametrize("name", ["fwd_pc", "rk_close_once"])
def test_fallbacks_keep_the_last_stage_on_the_full_list(graph, problem, name):
    """fwd_pc 0 (no dense kernel has the form) and rk_close_once 0 (no closing combination in the dense launch): the last
    stage runs on the full list - the isolated rows of S are written - and y(1) has the bits of diag_rows 0."""
    iso = graph[2]
    out = {}
    for rows in (1, 0):
        with options(**{"diag_rows": rows, "diag_last": 1, name: 0}):
            out[rows] = problem.forward(iso)
    assert torch.isfinite(out[1][0]).all() and torch.equal(out[1][0], out[0][0])
    assert out[1][1] == out[0][1]
    assert out[1][3] and out[0][3]
